"""GPU parity of the batched estimator entries with oracle/ransac_oracle.c: every problem of a gh_ransac_batch_dev /
gh_ransac_pairs_dev call returns the 12 model doubles, the mask and the inlier count of one single-problem RANSAC call on
its rows, bit for bit.  Problems below the sample size sit first, in the middle and last of the batches: every kernel has
to skip them before its sampler (which would not end).  Output buffers go in filled with 0xAB."""
import ctypes as C

import numpy as np
import pytest

import ransac_cases as rc

pytestmark = pytest.mark.gpu

SEED = 3
GH_ERR_ARG = 1  # include/gslam_hip.h


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(model):
    return np.zeros((0, rc.DIM_P[model])), np.zeros((0, rc.DIM_Q[model]))


def _upload(model, probs):
    """probs: [(P, Q)] -> (src, dst, offsets) on the device, offsets on the host."""
    dp, dq = rc.DIM_P[model], rc.DIM_Q[model]
    src = np.concatenate([np.asarray(P, np.float64).reshape(-1, dp) for P, _ in probs])
    dst = np.concatenate([np.asarray(Q, np.float64).reshape(-1, dq) for _, Q in probs])
    off = np.zeros(len(probs) + 1, np.int32)
    off[1:] = np.cumsum([len(P) for P, _ in probs])
    return _dev(src), _dev(dst), _dev(off), off


def _seed_tensor(seeds):
    return _dev(np.array(seeds, dtype=np.uint64).view(np.int64))


def _batch(ctx, model, probs, threshold=0.0, thresholds=None, seed=SEED, seeds=None):
    """gh_ransac_batch_dev on dirty output buffers -> (models n x 12, [mask of each problem], inliers) on the host."""
    import torch
    from gslam_amd import hip
    src, dst, off_d, off = _upload(model, probs)
    n = len(probs)
    thr_d = None if thresholds is None else _dev(np.asarray(thresholds, np.float64))
    seed_d = None if seeds is None else _seed_tensor(seeds)
    models = torch.full((n, 12), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((int(off[-1]),), 0xAB, dtype=torch.uint8, device="cuda")
    inliers = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    st = hip.lib.gh_ransac_batch_dev(ctx.h, model, _ptr(src), _ptr(dst), _ptr(off_d), n, C.c_double(threshold), _ptr(thr_d),
                                     C.c_uint64(seed), _ptr(seed_d), _ptr(models), _ptr(mask), _ptr(inliers))
    assert st == 0, (st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    mask = mask.cpu().numpy()
    return models.cpu().numpy(), [mask[off[p]:off[p + 1]] for p in range(n)], inliers.cpu().numpy()


def _same(got, p, want, key):
    gm, gmasks, gcnt = got
    em, emask, ecnt = want[:3]
    assert int(gcnt[p]) == ecnt, (key, int(gcnt[p]), ecnt)
    assert np.array_equal(gmasks[p], emask), (key, int(gmasks[p].sum()), int(emask.sum()))
    assert gm[p].tobytes() == em.tobytes(), (key, gm[p], em)


def _oracle(oracle, model, P, Q, thr, seed=SEED):
    return oracle.estimate_ex(model, P, Q, thr, rc.RANSAC, confidence=1.0, seed=seed)


def _class_batch(model):
    """Every class of ransac_cases that applies to the model, an empty problem first, in the middle and last."""
    items = [(name, rc.CLASSES[name](model, 0)) for name in rc.CLASSES]
    items = [(name, c) for name, c in items if c is not None]
    probs = [("empty_first",) + _empty(model) + (rc.THR[model], "no_model")]
    for k, (name, (P, Q, thr, expect)) in enumerate(items):
        if k == len(items) // 2:
            probs.append(("empty_middle",) + _empty(model) + (rc.THR[model], "no_model"))
        probs.append((name, P, Q, thr, rc.expect_for(expect, rc.RANSAC)))
    probs.append(("empty_last",) + _empty(model) + (rc.THR[model], "no_model"))
    return probs


def test_the_class_batches_cover_the_branches():
    """(no device work) over the eight models the batches of test_every_class_as_one_batch hold ties and both projection
    classes; every single one holds problems below the sample size."""
    labels = {m: {(name, e) for name, _, _, _, e in _class_batch(m)} for m in rc.MODELS}
    assert all(("n_s_minus_1", "no_model") in labels[m] for m in rc.MODELS)
    assert any(e == "ties" for m in rc.MODELS for _, e in labels[m])
    assert {("projection_underflow", "projection")} <= labels[4] and ("projection_failure", "no_model") in labels[4]
    for must in ("n_s_plus_0", "block_63", "block_513", "coincident", "collinear", "nonfinite_both", "thr_0", "thr_inf"):
        assert all(any(name == must for name, _ in labels[m]) for m in rc.MODELS), must
    assert any(name == "coplanar" for name, _ in labels[3])


@pytest.mark.parametrize("model", rc.MODELS)
def test_every_class_as_one_batch(ctx, oracle, model):
    probs = _class_batch(model)
    got = _batch(ctx, model, [(P, Q) for _, P, Q, _, _ in probs], thresholds=[thr for _, _, _, thr, _ in probs])
    seen = set()
    for p, (name, P, Q, thr, expect) in enumerate(probs):
        want = _oracle(oracle, model, P, Q, thr)
        _same(got, p, want, (model, name))
        if expect in ("no_model", "projection"):  # (a regular hypothesis that fits no row keeps its model: thr_0 can do that)
            assert want[2] == 0 and not want[0].any() and not got[0][p].any() and not got[1][p].any(), (model, name)
            seen.add(expect)
        if expect == "ties":
            assert want[2] > 0
            seen.add("ties")
    assert "no_model" in seen
    assert ("ties" in seen) == (model in (0, 1, 3, 6)), seen
    assert ("projection" in seen) == (model == 4), seen
    assert got[2][0] == got[2][-1] == 0  # the empty problems at both ends


@pytest.mark.parametrize("model", (0, 2, 6))
def test_tile_boundaries(ctx, oracle, model):
    from gslam_amd import estimator
    T = estimator.batch_tile_rows(model)
    assert T > 8
    sizes = (T - 1, 5, T, T + 1, 2 * T + 1)
    probs = [rc.nominal(model, n, seed=k)[:2] for k, n in enumerate(sizes)]
    got = _batch(ctx, model, probs, threshold=rc.THR[model])
    for p, (P, Q) in enumerate(probs):
        want = _oracle(oracle, model, P, Q, rc.THR[model])
        _same(got, p, want, (model, sizes[p]))
        assert want[2] > sizes[p] // 2 or sizes[p] == 5, (model, sizes[p], want[2])


def test_seeds_and_scalars(ctx, oracle):
    """Per-problem seeds through the mirror; then the scalar seed and threshold (seeds = thresholds = NULL), which equal
    the single-problem calls on the same context."""
    import torch
    from gslam_amd import estimator
    for model in rc.MODELS:
        P, Q, thr, _ = rc.CLASSES["nominal"](model, 0)
        probs = [(P, Q)] * len(rc.SEEDS)
        src, dst, off_d, off = _upload(model, probs)
        models, mask, inliers = estimator.estimate_batch(ctx, model, src, dst, off_d, 0.0, 0,
                                                         thresholds=_dev(np.full(len(probs), thr)), seeds=_seed_tensor(rc.SEEDS))
        torch.cuda.synchronize()
        got = (models.cpu().numpy(), [mask.cpu().numpy()[off[p]:off[p + 1]] for p in range(len(probs))], inliers.cpu().numpy())
        for p, seed in enumerate(rc.SEEDS):
            _same(got, p, _oracle(oracle, model, P, Q, thr, seed=seed), (model, seed))
        assert len({got[0][p].tobytes() for p in range(len(probs))}) > 1 or model == 6  # (the seeds do reach the sampler)
        got = _batch(ctx, model, probs, threshold=thr, seed=SEED)
        single = estimator.estimate(ctx, model, P, Q, thr, seed=SEED)
        for p in range(len(probs)):
            _same(got, p, single, (model, "scalar", p))
        _same(got, 0, _oracle(oracle, model, P, Q, thr), (model, "scalar vs oracle"))


# ---------------------------------------------------------------- the pair entry
CAP = 300
COUNTS = (0, 7, 300, 257)
PAIRS = ((0, 1), (1, 2), (2, 3), (3, 2), (2, 2))
PAIR_THR = {0: 2.0, 1: 2.0, 2: 1.0}


def _synthetic_frames(model):
    """Four frames of keypoints seen through a known homography / affinity / second camera, and the match rows of PAIRS:
    about 30 % wrong matches, -1 entries, entries >= counts[train] (inside and far outside the arrays), a keep mask with
    holes.  Rows past a frame's count hold coordinates nobody may read."""
    from gslam_amd.orb import KP_DTYPE
    rng = np.random.default_rng([77, model])
    kps = np.zeros((4, CAP), KP_DTYPE)
    kps["x"], kps["y"] = 1e9, -1e9
    kps["size"], kps["octave"], kps["class_id"] = 31.0, 0, -1
    if model == 2:
        X = np.c_[rng.uniform(-3, 3, (CAP, 2)), rng.uniform(4, 9, CAP)]
        th = 0.1
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        X2 = X @ R.T + np.array([0.5, 0.05, 0.1])
        a, b = 500 * X[:, :2] / X[:, 2:3] + (320, 240), 500 * X2[:, :2] / X2[:, 2:3] + (320, 240)
    else:
        a = rng.uniform((20, 20), (620, 460), (CAP, 2))
        H = np.array([[0.95, 0.04, 12.0], [-0.03, 1.02, -8.0], [0.0, 0.0, 1.0]])
        if model == 0:
            H[2, :2] = (2e-5, -1e-5)
        ah = np.c_[a, np.ones(CAP)] @ H.T
        b = ah[:, :2] / ah[:, 2:3]
    b = b + rng.normal(size=b.shape) * 0.3
    perm3 = rng.permutation(CAP)          # frame 3 holds the images of frame 2's points, shuffled; its count cuts some off
    where3 = np.argsort(perm3)            # frame 2 row i -> frame 3 row where3[i]
    kps["x"][2], kps["y"][2] = a[:, 0], a[:, 1]
    kps["x"][3], kps["y"][3] = b[perm3, 0], b[perm3, 1]
    kps["x"][1, :7], kps["y"][1, :7] = b[:7, 0], b[:7, 1]  # frame 1: the images of frame 2's first seven points
    counts = np.array(COUNTS, np.int32)
    idx1 = np.full((len(PAIRS), CAP), -1, np.int32)
    idx1[0] = rng.integers(0, 7, CAP)                      # pair (0, 1): the query frame is empty whatever the rows say
    idx1[1, :7] = np.arange(7)                             # pair (1, 2): at most seven correspondences
    idx1[1, 7:] = rng.integers(0, CAP, CAP - 7)
    idx1[2] = where3                                       # pair (2, 3): rows >= 257 appear by themselves
    idx1[3] = perm3                                        # pair (3, 2)
    idx1[4] = np.arange(CAP)                               # pair (2, 2): a frame against itself
    for p in (2, 3, 4):
        wrong = rng.random(CAP) < 0.3
        idx1[p, wrong] = rng.integers(0, CAP, int(wrong.sum()))
        idx1[p, rng.choice(CAP, 12, replace=False)] = -1
        idx1[p, rng.choice(CAP, 6, replace=False)] = (CAP, 65535, 2 ** 31 - 1, -2 ** 31, -7, 1 << 20)
    idx1[3, :257][rng.choice(257, 5, replace=False)] = 299
    idx1[1, 2] = -1
    keep = (rng.random((len(PAIRS), CAP)) < 0.85).astype(np.uint8)
    keep[1, :7] = (1, 1, 1, 0, 1, 1, 1)
    return kps, counts, idx1, keep


@pytest.mark.parametrize("model", (0, 1, 2))
@pytest.mark.parametrize("with_keep", (True, False))
def test_pairs_synthetic(ctx, oracle, model, with_keep):
    import torch
    from gslam_amd import estimator, hip
    kps, counts, idx1, keep = _synthetic_frames(model)
    if not with_keep:
        keep = None
    pair_q, pair_t = (np.array([p[k] for p in PAIRS], np.int32) for k in (0, 1))
    corr = estimator.correspondences_from_matches(kps, counts, pair_q, pair_t, idx1, keep)
    P = len(PAIRS)
    d_kps = _dev(kps.view(np.float32).reshape(4, CAP, 7))
    d_counts, d_pq, d_pt, d_idx1 = _dev(counts), _dev(pair_q), _dev(pair_t), _dev(idx1)
    d_keep = None if keep is None else _dev(keep)
    models = torch.full((P, 12), 7.0, dtype=torch.float64, device="cuda")
    inlier = torch.full((P, CAP), 0xAB, dtype=torch.uint8, device="cuda")
    n_corr = torch.full((P,), -5, dtype=torch.int32, device="cuda")
    inliers = torch.full((P,), -5, dtype=torch.int32, device="cuda")
    st = hip.lib.gh_ransac_pairs_dev(ctx.h, model, _ptr(d_kps), _ptr(d_counts), CAP, _ptr(d_pq), _ptr(d_pt), P, _ptr(d_idx1),
                                     _ptr(d_keep), C.c_double(PAIR_THR[model]), C.c_uint64(SEED), _ptr(models), _ptr(inlier),
                                     _ptr(n_corr), _ptr(inliers))
    assert st == 0, hip.lib.gh_last_error(ctx.h)
    torch.cuda.synchronize()
    models, inlier, n_corr, inliers = (t.cpu().numpy() for t in (models, inlier, n_corr, inliers))
    assert n_corr.tolist() == [len(r) for _, _, r in corr]
    assert n_corr[0] == 0 and 0 < n_corr[1] <= 6 and n_corr[2] > 100 and n_corr[3] > 100
    saw_model = saw_none = False
    for p, (src, dst, rows) in enumerate(corr):
        em, emask, ecnt, _ = _oracle(oracle, model, src, dst, PAIR_THR[model])
        want = np.zeros(CAP, np.uint8)
        want[rows[emask.astype(bool)]] = 1
        assert int(inliers[p]) == ecnt, (model, p, int(inliers[p]), ecnt)
        assert models[p].tobytes() == em.tobytes(), (model, p, models[p], em)
        assert np.array_equal(inlier[p], want), (model, p, int(inlier[p].sum()), int(want.sum()))
        if len(rows) < rc.S_OF[model]:
            assert ecnt == 0 and not models[p].any() and not inlier[p].any()
            saw_none = True
        saw_model = saw_model or ecnt > 100
    assert saw_model and saw_none
    if with_keep and model == 0:  # the mirror makes the same call
        got = estimator.estimate_pairs(ctx, model, d_kps, d_counts, d_pq, d_pt, d_idx1, d_keep, PAIR_THR[model], SEED)
        torch.cuda.synchronize()
        for g, w in zip(got, (models, inlier, n_corr, inliers)):
            assert g.cpu().numpy().tobytes() == w.tobytes()


def test_pairs_end_to_end(ctx):
    """Synthetic frames -> ORB -> pair matcher -> match mask -> gh_ransac_pairs_dev (F), everything on the device; the
    result equals gh_ransac_estimate per pair on the downloaded rows."""
    import torch
    from gslam_amd import estimator
    from gslam_amd.matcher import BFMatcher
    from gslam_amd.orb import OrbExtractor, kps_to_numpy, synth_frames
    ex = OrbExtractor(ctx, 640, 480, max_batch=4, n_features=500)
    frames = synth_frames(ctx, 4, 640, 480, base_seed=0x5EED0000)
    kps, desc, counts = ex.extract(frames)
    cap = kps.shape[1]
    pq = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    pt = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device="cuda")
    m = BFMatcher(ctx)
    idx1, d1, d2 = m.match_pairs(desc, counts, pq, pt)
    keep = m.mask(idx1.view(-1), d1.view(-1), d2.view(-1), max_dist=80)
    models, inlier, n_corr, inliers = estimator.estimate_pairs(ctx, estimator.FUNDAMENTAL, kps, counts, pq, pt, idx1, keep, 1.0, SEED)
    torch.cuda.synchronize()
    corr = estimator.correspondences_from_matches(kps_to_numpy(kps), counts.cpu().numpy(), pq.cpu().numpy(), pt.cpu().numpy(),
                                                  idx1.cpu().numpy(), keep.cpu().numpy())
    models, inlier, n_corr, inliers = (t.cpu().numpy() for t in (models, inlier, n_corr, inliers))
    assert inlier.shape == (4, cap)
    assert n_corr.tolist() == [len(r) for _, _, r in corr] and n_corr.max() >= 8
    for p, (src, dst, rows) in enumerate(corr):
        em, emask, ecnt = estimator.estimate(ctx, estimator.FUNDAMENTAL, src, dst, 1.0, seed=SEED)
        want = np.zeros(cap, np.uint8)
        want[rows[emask.astype(bool)]] = 1
        assert int(inliers[p]) == ecnt and models[p].tobytes() == em.tobytes() and np.array_equal(inlier[p], want), p
    ex.close()


def test_call_sequence_independence(ctx, oracle):
    """The scratch block is reused and only partly overwritten: a batch with a problem of 2 T + 1 rows, a one-problem batch
    of three rows, and the first again return identical bytes each time."""
    from gslam_amd import estimator
    T = estimator.batch_tile_rows(1)
    big = [rc.nominal(1, 2 * T + 1)[:2], rc.nominal(1, 40, seed=1)[:2], _empty(1)]
    small = [rc.nominal(1, 3)[:2]]
    a = _batch(ctx, 1, big, threshold=rc.THR[1])
    b = _batch(ctx, 1, small, threshold=rc.THR[1])
    c = _batch(ctx, 1, big, threshold=rc.THR[1])
    d = _batch(ctx, 1, small, threshold=rc.THR[1])
    for x, y in ((a, c), (b, d)):
        assert x[0].tobytes() == y[0].tobytes() and x[2].tobytes() == y[2].tobytes()
        assert all(np.array_equal(u, v) for u, v in zip(x[1], y[1]))
    _same(b, 0, _oracle(oracle, 1, small[0][0], small[0][1], rc.THR[1]), "small")
    assert b[2][0] == 3  # (three rows are exactly an affine sample: a model that fits them)
    for p, (P, Q) in enumerate(big):
        _same(a, p, _oracle(oracle, 1, P, Q, rc.THR[1]), ("big", p))


def test_refusals(ctx, oracle):
    import torch
    from gslam_amd import hip
    P, Q, thr = rc.nominal(0, 50)
    src, dst, off_d, off = _upload(0, [(P, Q), (P[:3], Q[:3])])
    models = torch.full((2, 12), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((53,), 0xAB, dtype=torch.uint8, device="cuda")
    inliers = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    thrs = _dev(np.array([thr, thr]))

    def call(model=0, n=2, t=thr, src=src, dst=dst, off=off_d, thrs=None, models=models, inliers=inliers):
        return hip.lib.gh_ransac_batch_dev(ctx.h, model, _ptr(src), _ptr(dst), _ptr(off), n, C.c_double(t), _ptr(thrs),
                                           C.c_uint64(SEED), None, _ptr(models), _ptr(mask), _ptr(inliers))

    assert call() == 0
    for kw in (dict(model=-1), dict(model=8), dict(n=-1), dict(src=None), dict(dst=None), dict(off=None), dict(models=None),
               dict(inliers=None), dict(t=-1.0), dict(t=float("nan"))):
        assert call(**kw) == GH_ERR_ARG, kw
    assert call(n=0) == 0 and call(n=0, src=None) == 0   # nothing to do is no error
    assert call(t=-1.0, thrs=thrs) == 0                  # the scalar is not read when every problem brings its own
    assert hip.lib.gh_ransac_batch_dev(None, 0, _ptr(src), _ptr(dst), _ptr(off_d), 2, C.c_double(thr), None, C.c_uint64(SEED), None,
                                       _ptr(models), _ptr(mask), _ptr(inliers)) == GH_ERR_ARG
    # a per-problem threshold that is negative or NaN is "no model" for that problem alone
    got = _batch(ctx, 0, [(P, Q), (P, Q), (P, Q)], thresholds=[-1.0, thr, float("nan")])
    want = _oracle(oracle, 0, P, Q, thr)
    _same(got, 1, want, "good threshold")
    assert want[2] > 25
    for p in (0, 2):
        assert got[2][p] == 0 and not got[0][p].any() and not got[1][p].any()
    # offsets that are not monotone: the reversed range is 0 rows, its neighbours are untouched
    bad = _dev(np.array([0, 50, 40, 53], np.int32))
    assert call(off=bad, n=3, models=torch.zeros((3, 12), dtype=torch.float64, device="cuda"),
                inliers=(cnt := torch.full((3,), -5, dtype=torch.int32, device="cuda"))) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().numpy()[1] == 0 and cnt.cpu().numpy()[0] == want[2]

    # the pair entry: models other than H / A2 / F, a cap past 65535, NULL arrays
    k = torch.zeros((2, 8, 7), dtype=torch.float32, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    cts, pq, pt, idx = i32(8, 8), i32(0), i32(1), torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    om, oi, oc, on = (torch.zeros((1, 12), dtype=torch.float64, device="cuda"), torch.zeros((1, 8), dtype=torch.uint8, device="cuda"),
                      i32(0), i32(0))

    def pcall(model=0, cap=8, npairs=1, kps=k, t=2.0, inl=oi):
        return hip.lib.gh_ransac_pairs_dev(ctx.h, model, _ptr(kps), _ptr(cts), cap, _ptr(pq), _ptr(pt), npairs, _ptr(idx), None,
                                           C.c_double(t), C.c_uint64(SEED), _ptr(om), _ptr(inl), _ptr(oc), _ptr(on))

    assert pcall() == 0
    for kw in (dict(model=3), dict(model=4), dict(model=7), dict(model=-1), dict(cap=65536), dict(cap=-1), dict(npairs=-1),
               dict(kps=None), dict(inl=None), dict(t=-1.0), dict(t=float("nan"))):
        assert pcall(**kw) == GH_ERR_ARG, kw
    assert pcall(npairs=0) == 0
    assert call() == 0 and pcall() == 0  # the context is usable after a refusal
    torch.cuda.synchronize()
