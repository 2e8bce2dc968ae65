"""GPU parity of the BoW kernels (bow_words_kernel, bow_words_f32_kernel, bow_assemble_kernel, bow_score_kernel, through the
C ABI) with oracle/bow_oracle.c on the adversarial classes of tests/bow_cases.py.  tests/test_bow_adversarial_oracle.py
shows on the CPU that each class reaches what it names and that the oracle equals the reference there; here word, node,
weight, BoW ids and bow_n are equal and the BoW floats bit-identical, the padding is the documented 0xFFFFFFFF / 0.0, and
the scores are bit-identical doubles except KL (logf: 1e-6 relative to max(1, |e|)).  The entry points' limits (cap,
n_images, counts, descriptor widths) run at their edges and one step past, where they must refuse and stay usable.

No case reads or writes out of bounds: every buffer passed has the full n_images x cap extent of the call, counts outside
[0, cap] are clamped by the kernels (min(count, cap); a negative count is an empty image), and refused calls return before
any launch."""
import ctypes as C
import os

import numpy as np
import pytest

import bow_cases as bc
import bow_restate as br
from gslam_amd import bow_synth

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
NONE = 0xFFFFFFFF
KL_REL = 1e-6   # gslam_amd/csrc/bow_score.hip:16-17
GOLD = os.path.join(os.path.dirname(__file__), "golden", "bow_adversarial.npz")

_expected = {}


def expected(oracle, name, levelsup):
    """The oracle's outputs for a class, computed once and shared (read only)."""
    if (name, levelsup) not in _expected:
        voc, desc, _, _ = bc.case(name)
        _expected[name, levelsup] = oracle.bow_transform(voc, desc, levelsup)
    return _expected[name, levelsup]


def _same_transform(got, want, key):
    for g, w, what in zip(got, want, ("word", "weight", "node", "bow ids", "bow values")):
        assert len(g) == len(w) and g.tobytes() == w.tobytes(), (key, what, int((np.asarray(g) != np.asarray(w)).sum()))


def _batched(v, desc, counts, levelsup):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
    c = None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    out = v.transform(d, c, levelsup=levelsup)
    torch.cuda.synchronize()
    word, weight, node, bw, bv, bn = [t.cpu().numpy() for t in out]
    return word.view(np.uint32), weight, node.view(np.uint32), bw.view(np.uint32), bv, bn


def _check_image(got, b, n, want, key):
    """Image b of a batched call against the oracle's outputs for its first n features, padding included."""
    word, weight, node, bw, bv, bn = got
    nb = len(want[3])
    assert bn[b] == nb, (key, b, int(bn[b]), nb)
    _same_transform((word[b, :n], weight[b, :n], node[b, :n], bw[b, :nb], bv[b, :nb]), want, (key, b))
    assert (word[b, n:] == NONE).all() and not weight[b, n:].any() and (node[b, n:] == NONE).all(), (key, b)
    assert (bw[b, nb:] == NONE).all() and bv[b, nb:].tobytes() == bytes(4 * (bv.shape[1] - nb)), (key, b)


# ------------------------------------------------------------------------------------------------------- transform
@pytest.mark.parametrize("name", list(bc.CLASSES))
def test_class_parity_host_entry(ctx, oracle, name):
    from gslam_amd.bow import Vocabulary
    voc, desc, levelsups, _ = bc.case(name)
    v = Vocabulary(ctx, voc)
    for levelsup in levelsups:
        _same_transform(v.transform_host(desc, levelsup), expected(oracle, name, levelsup), (name, levelsup))
    v.close()


def _groups():
    by_voc = {}
    for name in bc.CLASSES:
        by_voc.setdefault(bc.voc_key(bc.case(name)[0]), []).append(name)
    return ["+".join(names) for names in by_voc.values()]


@pytest.mark.parametrize("group", _groups())
def test_class_parity_batched(ctx, oracle, group):
    """The classes that share a vocabulary ride as ragged images of one call, followed by an empty image, an image whose
    count is above the capacity (clamped to cap) and one whose count is negative (empty)."""
    from gslam_amd.bow import Vocabulary
    names = group.split("+")
    voc, _, levelsups, _ = bc.case(names[0])
    sets = [bc.case(n)[1] for n in names]
    cap = max(len(d) for d in sets)
    desc = np.zeros((len(sets) + 3, cap) + sets[0].shape[1:], sets[0].dtype)
    for b, d in enumerate(sets):
        desc[b, :len(d)] = d
    full = np.resize(sets[0], (cap,) + sets[0].shape[1:])  # the first set repeated to cap rows
    desc[len(sets):] = full
    counts = [len(d) for d in sets] + [0, cap + 7, -3]
    v = Vocabulary(ctx, voc)
    for levelsup in levelsups:
        got = _batched(v, desc, counts, levelsup)
        for b, n in enumerate(names):
            _check_image(got, b, counts[b], expected(oracle, n, levelsup), (n, levelsup))
        empty = oracle.bow_transform(voc, full[:0], levelsup)
        _check_image(got, len(sets), 0, empty, (group, "empty"))
        _check_image(got, len(sets) + 1, cap, oracle.bow_transform(voc, full, levelsup), (group, "count > cap"))
        _check_image(got, len(sets) + 2, 0, empty, (group, "negative count"))
    v.close()
    if len(names) > 1:
        assert len({len(d) for d in sets}) > 1  # ragged


@pytest.mark.parametrize("name", bc.FIXTURE_CLASSES)
def test_class_parity_with_recorded_reference(ctx, name):
    """Directly against the reference's recorded outputs (no oracle in between).  The node id is compared where the
    reference defines it and is the contract's 0 at the shallow leaves (include/gslam_hip.h, gh_bow_transform_dev)."""
    from gslam_amd.bow import Vocabulary
    g = np.load(GOLD)
    voc, _, levelsups, _ = bc.case(name)
    v = Vocabulary(ctx, voc)
    for levelsup in levelsups:
        word, weight, node, bw, bv = v.transform_host(g[f"{name}/desc"], levelsup)
        defined = g[f"{name}/defined_{levelsup}"]
        assert np.array_equal(word, g[f"{name}/word"]) and weight.tobytes() == g[f"{name}/weight"].tobytes()
        assert np.array_equal(bw, g[f"{name}/bow_ids"]) and bv.tobytes() == g[f"{name}/bow_vals"].tobytes()
        assert np.array_equal(node[defined], g[f"{name}/node_{levelsup}"][defined]) and not node[~defined].any()
    v.close()


@pytest.mark.parametrize("cap", [1, 255, 256, 257, 16384])
def test_capacity_edges(ctx, oracle, cap):
    """cap at 1, around the smallest sort size (P = 256 -> 512) and at the largest (P = 16384, 128 KB of LDS)."""
    from gslam_amd.bow import Vocabulary
    voc = bow_synth.make_vocabulary(k=10, L=3, seed=5, weighting=bow_synth.TF_IDF, scoring=bow_synth.L2_NORM, stop_frac=0.05)
    desc = np.stack([bow_synth.features_near_words(voc, cap, seed=50 + b) for b in range(3)])
    counts = [cap, cap - 1, (cap + 1) // 2]
    v = Vocabulary(ctx, voc)
    got = _batched(v, desc, counts, 1)
    for b in range(3):
        _check_image(got, b, counts[b], oracle.bow_transform(voc, desc[b, :counts[b]], 1), (cap, b))
    got = _batched(v, desc, None, 1)  # no counts: cap rows each
    for b in range(3):
        _check_image(got, b, cap, oracle.bow_transform(voc, desc[b], 1), (cap, b, "no counts"))
    v.close()


def test_65535_images(ctx, oracle):
    """The largest grid.y: 65535 one-feature images.  A one-feature image under TF_IDF / DOT is (word: weight / 1) when the
    word is not stopped; the per-feature outputs come from one oracle call and 50 images are checked against it whole."""
    from gslam_amd.bow import Vocabulary
    B = 65535
    voc = bow_synth.make_vocabulary(k=6, L=3, seed=8, weighting=bow_synth.TF_IDF, scoring=bow_synth.DOT_PRODUCT, stop_frac=0.1)
    desc = bow_synth.features_near_words(voc, B, seed=9)
    v = Vocabulary(ctx, voc)
    word, weight, node, bw, bv, bn = _batched(v, desc[:, None, :], None, 1)
    v.close()
    e_word, e_weight, e_node, _, _ = oracle.bow_transform(voc, desc, 1)
    assert np.array_equal(word[:, 0], e_word) and weight[:, 0].tobytes() == e_weight.tobytes() and np.array_equal(node[:, 0], e_node)
    kept = e_weight > 0
    assert kept.any() and (~kept).any()
    assert np.array_equal(bn, kept.astype(np.int32))
    assert np.array_equal(bw[:, 0], np.where(kept, e_word, NONE)) and bv[:, 0].tobytes() == np.where(kept, e_weight, np.float32(0)).tobytes()
    for b in [0, B - 1] + np.random.default_rng(1).integers(0, B, 48).tolist():
        e = oracle.bow_transform(voc, desc[b:b + 1], 1)
        assert bn[b] == len(e[3]) and np.array_equal(bw[b, :bn[b]], e[3]) and bv[b, :bn[b]].tobytes() == e[4].tobytes()


def _create_status(ctx, voc, desc_bytes=None, dims=None, **over):
    """gh_bow_vocab_create_bytes / _f32 on a vocabulary dict with single arguments overridden -> status."""
    from gslam_amd import hip
    a = dict(k=int(voc["k"]), L=int(voc["L"]), weighting=int(voc["weighting"]), scoring=int(voc["scoring"]),
             nodes=np.ascontiguousarray(voc["nodes"]), desc=np.ascontiguousarray(voc["desc"]))
    a.update(over)
    h = C.c_void_p()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)
    if dims is not None:
        st = hip.lib.gh_bow_vocab_create_f32(ctx.h, a["k"], a["L"], a["weighting"], a["scoring"], len(a["nodes"]), pv(a["nodes"]),
                                             pv(a["desc"]), dims, C.byref(h))
    else:
        st = hip.lib.gh_bow_vocab_create_bytes(ctx.h, a["k"], a["L"], a["weighting"], a["scoring"], len(a["nodes"]),
                                               pv(a["nodes"]), pv(a["desc"]), desc_bytes or a["desc"].shape[1], C.byref(h))
    if st == 0:
        hip.lib.gh_bow_vocab_destroy(h)
    else:
        assert not h.value
    return st


def test_refusals_leave_the_context_usable(ctx, oracle):
    import torch
    from gslam_amd import bow, hip
    voc = bow_synth.make_vocabulary(k=4, L=2, seed=6)
    fvoc = bow_synth.make_float_vocabulary(k=3, L=2, dims=8, seed=6)
    assert _create_status(ctx, voc) == 0 and _create_status(ctx, fvoc, dims=8) == 0
    wide = dict(voc, desc=np.zeros((len(voc["nodes"]), 16392), np.uint8))     # the buffers cover what each call names
    fwide = dict(fvoc, desc=np.zeros((len(fvoc["nodes"]), 4104), np.float32))
    assert _create_status(ctx, wide, desc_bytes=12) == GH_ERR_ARG
    assert _create_status(ctx, wide, desc_bytes=16392) == GH_ERR_ARG
    assert _create_status(ctx, wide, desc_bytes=16384) == 0
    assert _create_status(ctx, fwide, dims=4) == GH_ERR_ARG
    assert _create_status(ctx, fwide, dims=4104) == GH_ERR_ARG
    assert _create_status(ctx, fwide, dims=4096) == 0
    too_many = voc["nodes"].copy()
    too_many["childNum"][1] = voc["k"] + 1
    assert _create_status(ctx, voc, nodes=too_many) == GH_ERR_ARG
    past_end = voc["nodes"].copy()
    past_end["childNum"][len(past_end) - 1] = 1  # a last-level node with a child: p * k + 1 is past nnodes
    assert _create_status(ctx, voc, nodes=past_end) == GH_ERR_ARG
    for key, bad in (("weighting", -1), ("weighting", 4), ("scoring", -1), ("scoring", 6)):
        assert _create_status(ctx, voc, **{key: bad}) == GH_ERR_ARG, (key, bad)

    v = bow.Vocabulary(ctx, voc)
    p = lambda t: C.c_void_p(t.data_ptr())

    def transform_status(n_images, cap):
        desc = torch.zeros((n_images, cap, 32), dtype=torch.uint8, device="cuda")
        out = v.alloc(n_images, cap)
        return hip.lib.gh_bow_transform_dev(v.h, p(desc), None, cap, n_images, 1, *[p(t) for t in out])

    assert transform_status(65536, 1) == GH_ERR_ARG
    assert transform_status(1, 16385) == GH_ERR_ARG
    assert transform_status(2, 3) == 0
    big = np.zeros((16385, 32), np.uint8)
    with pytest.raises(hip.GslamHipError):
        v.transform_host(big, 1)
    ids = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    vals = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    for sc in (-1, 6):
        assert hip.lib.gh_bow_score_dev(ctx.h, sc, p(ids), p(vals), p(cnt), 1, 4, p(ids), p(vals), p(cnt), 1, 4, p(out)) == GH_ERR_ARG
        with pytest.raises(hip.GslamHipError):
            bow.score_host(ctx, sc, (np.zeros(1, np.uint32), np.ones(1, np.float32)), [(np.zeros(1, np.uint32), np.ones(1, np.float32))])
    # the context and the vocabulary still work
    desc = bow_synth.features_near_words(voc, 100, seed=7)
    _same_transform(v.transform_host(desc, 1), oracle.bow_transform(voc, desc, 1), "after refusals")
    v.close()


# ---------------------------------------------------------------------------------------------------------- scoring
def _same_scores(scoring, got, want, key):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, key
    ok = (got == want) | (np.isnan(got) & np.isnan(want))
    if scoring == 3:
        with np.errstate(invalid="ignore"):
            ok |= np.abs(got - want) <= KL_REL * np.maximum(1.0, np.abs(want))
    assert ok.all(), (key, np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])


def _score_gpu(ctx, scoring, q, db):
    import torch
    from gslam_amd import bow
    up = lambda v: (torch.from_numpy(v[0].view(np.int32)).cuda(), torch.from_numpy(v[1]).cuda(), torch.from_numpy(v[2]).cuda())
    S = bow.score(ctx, scoring, up(q), up(db))
    torch.cuda.synchronize()
    return S.cpu().numpy()


@pytest.mark.parametrize("name", [n for n in bc.SCORE_CLASSES if n != "nq_65537"])
def test_score_class_parity(ctx, oracle, name):
    from gslam_amd import bow
    scoring, q, db, _ = bc.score_case(name)
    qe, de = br.effective(q), br.effective(db)
    want = np.array([[oracle.bow_score(scoring, a, b) for b in de] for a in qe])
    _same_scores(scoring, _score_gpu(ctx, scoring, q, db), want, name)
    _same_scores(scoring, bow.score_host(ctx, scoring, qe[0], de), want[0], (name, "host entry"))
    if q[0].shape[1] <= 200:  # the database side as the query side as well (KL is not symmetric)
        want = np.array([[oracle.bow_score(scoring, a, b) for b in qe] for a in de])
        _same_scores(scoring, _score_gpu(ctx, scoring, db, q), want, (name, "swapped"))


def test_score_65537_queries(ctx, oracle):
    """n_q above one launch's grid.y: the second launch's rows land at q0 * n_db.  Compared with the vectorised numpy
    restatement (tests/bow_restate.py) on all 65537 x 5 pairs, and with the oracle on both ends of each launch and a sample."""
    scoring, q, db, _ = bc.score_case("nq_65537")
    S = _score_gpu(ctx, scoring, q, db)
    _same_scores(scoring, S, br.score_all_pairs_symmetric(scoring, q, db), "nq_65537")
    qe, de = br.effective(q), br.effective(db)
    rows = sorted({0, 1, 65534, 65535, 65536} | set(np.random.default_rng(5).integers(0, len(qe), 45).tolist()))
    want = np.array([[oracle.bow_score(scoring, qe[i], b) for b in de] for i in rows])
    _same_scores(scoring, S[rows], want, "nq_65537 sample")
    assert np.count_nonzero(S[65535:]) > 0 and np.count_nonzero(S) > S.size // 4


# ------------------------------------------------------------------------------------------------------------- fuzz
def test_fuzz_random_trees(ctx, oracle):
    """Random small trees with early leaves, stopped words, every weighting / scoring, binary and float descriptors: three
    ragged images through the batched transform, then every image scored against every image."""
    from hypothesis import given, settings, strategies as st
    from gslam_amd.bow import Vocabulary

    @settings(max_examples=40, deadline=None)
    @given(k=st.integers(2, 6), L=st.integers(1, 4), leaf_frac=st.floats(0, 0.5), stop_frac=st.floats(0, 0.5),
           weighting=st.integers(0, 3), scoring=st.integers(0, 5),
           width=st.sampled_from([(8, False), (24, False), (32, False), (64, False), (8, True), (16, True)]),
           n=st.integers(0, 600), up=st.integers(0, 5), seed=st.integers(0, 2 ** 31 - 1))
    def run(k, L, leaf_frac, stop_frac, weighting, scoring, width, n, up, seed):
        rng = np.random.default_rng(seed)
        levelsup = min(up, L + 1)
        voc = bc.random_tree(rng, k, L, leaf_frac, stop_frac, weighting, scoring, *width)
        cap = max(n, 1)
        desc = np.stack([bc.random_features(rng, voc, cap) for _ in range(3)])
        counts = [n, int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1))]
        v = Vocabulary(ctx, voc)
        got = _batched(v, desc, counts, levelsup)
        v.close()
        key = (k, L, weighting, scoring, width, n, levelsup, seed)
        want = [oracle.bow_transform(voc, desc[b, :counts[b]], levelsup) for b in range(3)]
        for b in range(3):
            _check_image(got, b, counts[b], want[b], key)
        vec = (got[3], got[4], got[5])
        e = np.array([[oracle.bow_score(scoring, (a[3], a[4]), (b[3], b[4])) for b in want] for a in want])
        _same_scores(scoring, _score_gpu(ctx, scoring, vec, vec), e, key)

    run()
