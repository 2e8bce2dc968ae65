"""Adversarial inputs for the BoW transform and the six scorings: the classes that bow_synth's generators never produce
(tests/test_bow_adversarial_oracle.py takes the census of what each class reaches and pins the oracle on it,
tests/test_bow_adversarial_gpu.py holds the kernels to the oracle).  numpy only, seeded.

CLASSES[name]() -> (voc, desc, levelsups, expect)
    voc        the dict layout of bow_synth.make_vocabulary (k, L, weighting, scoring, nodes, desc)
    desc       n x desc_bytes uint8, or n x dims float32 for a float vocabulary
    levelsups  the `levelsup` values the class is run at
    expect     what the class was built to reach (the census asserts it with the restatement of tests/bow_restate.py):
               "nb": BoW length;  "shallow": (min share ending above level L - levelsup, min share reaching it) at
               levelsup 0 and 1;  "ties": (min share meeting a tie, min share won by a later child, min share won by the
               first child);  "stops_at": the non-leaf words a non-finite descent ends on;  "reference": False where
               the reference does not terminate and the class is never sent to it
SCORE_CLASSES[name]() -> (scoring, q, db, expect)
    q, db      (ids n x cap uint32 ascending per row, values n x cap float32, counts n int32) in the padded layout
    expect     "q_len" / "db_len": effective lengths;  "common": n_q x n_db intersection sizes;  "zeros": zero values occur
               among the common words of the query / the database side
Builders are cached: the arrays are shared and must not be written to."""
import functools

import numpy as np

from gslam_amd import bow_synth

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1, L2, CHI2, KL, BHATT, DOT = range(6)
NONE = 0xFFFFFFFF

CLASSES = {}
SCORE_CLASSES = {}
FIXTURE_CLASSES = ("shallow_leaves", "planted_ties_32", "one_word_257", "all_stopped")  # recorded in golden/bow_adversarial.npz


def _register(table, name):
    def deco(fn):
        table[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def _level_ranges(k, L):
    """[(first id, one past the last id)] of levels 0..L of a full k-ary tree stored as p*k+1 .. p*k+k."""
    out, s = [], 0
    for lvl in range(L + 1):
        out.append((s, s + k ** lvl))
        s += k ** lvl
    return out


def _reachable(voc):
    k, cn = voc["k"], voc["nodes"]["childNum"]
    seen, stack = [], [0]
    while stack:
        p = stack.pop()
        seen.append(p)
        stack.extend(range(p * k + 1, p * k + 1 + int(cn[p])))
    return np.array(sorted(seen))


def _reachable_leaves(voc):
    r = _reachable(voc)
    return r[voc["nodes"]["childNum"][r] == 0]


def _near(voc, ids, rng, flip_bits):
    d = voc["desc"][ids].copy()
    if flip_bits:
        flips = np.zeros((len(ids), 8 * d.shape[1]), np.uint8)
        np.put_along_axis(flips, rng.integers(0, 8 * d.shape[1], (len(ids), flip_bits)), 1, axis=1)
        d ^= np.packbits(flips, axis=1, bitorder="little")
    return d


def _hand_voc(k, L, child_num, weight, desc, weighting=TF_IDF, scoring=L1):
    nodes = np.zeros(len(child_num), dtype=[("childNum", "<u4"), ("weight", "<f4")])
    nodes["childNum"] = child_num
    nodes["weight"] = weight
    return {"k": k, "L": L, "weighting": weighting, "scoring": scoring, "nodes": nodes, "desc": desc}


# ---------------------------------------------------------------------------------------------------- transform classes
@_register(CLASSES, "shallow_leaves")
def shallow_leaves():
    """About 30 % of the level-1 and level-2 nodes and 15 % of level 3 are leaves with positive weights: the descent ends
    above level L - levelsup for many features, and the node output is the contract's 0 there."""
    rng = np.random.default_rng(101)
    voc = bow_synth.make_vocabulary(k=6, L=4, seed=101, scoring=L1)
    lv = _level_ranges(6, 4)
    nodes = voc["nodes"]
    for lvl, frac in ((1, 0.3), (2, 0.3), (3, 0.15)):
        ids = np.arange(*lv[lvl])
        cut = ids[rng.random(len(ids)) < frac]
        nodes["childNum"][cut] = 0
        nodes["weight"][cut] = rng.uniform(0.5, 9.0, len(cut)).astype(np.float32)
    leaves = _reachable_leaves(voc)
    shallow = leaves[leaves < lv[4][0]]
    desc = np.concatenate([_near(voc, rng.choice(shallow, 400), rng, 10), _near(voc, rng.choice(leaves, 400), rng, 10),
                           rng.integers(0, 256, (200, 32), dtype=np.uint8)])
    return voc, desc, (0, 1, 2, 4, 7), {"shallow": (0.10, 0.10)}


def _even_children(voc):
    """Make every pair of siblings differ in an even number of bits (a feature can then sit exactly between them)."""
    k, desc, cn = voc["k"], voc["desc"], voc["nodes"]["childNum"]
    for p in np.nonzero(cn)[0]:
        kids = np.arange(p * k + 1, p * k + 1 + int(cn[p]))
        odd = np.unpackbits(desc[kids] ^ desc[kids[0]], axis=1).sum(axis=1) & 1
        desc[kids[odd == 1], 0] ^= 1


def _between(a, others, rng):
    """A descriptor at exactly the same Hamming distance from `a` and from each of `others` (one or two rows): flip half
    of the bits in which each other row differs from a, sharing half of the bits in which both differ."""
    A = np.unpackbits(a)
    B = np.unpackbits(others[0]) ^ A
    C = np.unpackbits(others[1]) ^ A if len(others) > 1 else np.zeros_like(B)
    z = np.nonzero(B & C)[0]
    x = np.nonzero(B & ~C & 1)[0]
    y = np.nonzero(C & ~B & 1)[0]
    fz = len(z) // 2
    fx, fy = int(B.sum()) // 2 - fz, int(C.sum()) // 2 - fz
    F = np.concatenate([rng.permutation(z)[:fz], rng.permutation(x)[:fx], rng.permutation(y)[:fy]])
    A[F] ^= 1
    return np.packbits(A)


def _planted_ties(desc_bytes, seed):
    """For 60 % of the features two or three children of a node on the path are at exactly the same Hamming distance.
    The tied set is {0, j}, {0, i, j}, {i, j} or {i, j, k-1}: the first strict minimum takes child 0 or a middle child;
    the last child is often in the tied set and, by that rule, never the winner."""
    rng = np.random.default_rng(seed)
    k, L = 5, 3
    voc = bow_synth.make_vocabulary(k=k, L=L, seed=seed, ragged=False, desc_bytes=desc_bytes)
    _even_children(voc)
    lv = _level_ranges(k, L)
    n, out = 500, []
    for i in range(n):
        if i % 5 >= 3:
            out.append(_near(voc, rng.integers(lv[L][0], lv[L][1], 1), rng, 6)[0])
            continue
        p = int(rng.integers(0, lv[L][0]))  # an internal node on any level
        first = p * k + 1
        tied = [(0, 4), (0, 2, 3), (1, 3), (2, 3, 4), (1, 4), (0, 1)][i % 6]
        rows = voc["desc"][[first + c for c in tied]]
        out.append(_between(rows[0], rows[1:], rng))
    return voc, np.stack(out), (0, 1, 3), {"ties": (0.20, 0.05, 0.05)}


for _w, _s in ((32, 201), (64, 202), (24, 203)):
    _register(CLASSES, f"planted_ties_{_w}")(functools.partial(_planted_ties, _w, _s))


@_register(CLASSES, "duplicate_children")
def duplicate_children():
    """Half of the internal nodes carry a later child whose descriptor is a copy of an earlier one (its subtree and weights
    differ): every feature that comes by meets an exact tie, and features drawn from under the copy must still go to the
    original."""
    rng = np.random.default_rng(301)
    k, L = 5, 3
    voc = bow_synth.make_vocabulary(k=k, L=L, seed=301, ragged=False, scoring=L2)
    lv = _level_ranges(k, L)
    for p in range(lv[L][0]):
        if p % 2 == 0:
            i, j = [(0, 3), (2, 4), (1, 2)][p % 3]
            voc["desc"][p * k + 1 + j] = voc["desc"][p * k + 1 + i]
    desc = _near(voc, rng.integers(lv[L][0], lv[L][1], 600), rng, 8)
    return voc, desc, (0, 1), {"ties": (0.20, 0.05, 0.05)}


def _dyadic_float_voc(k, L, dims, seed, **kw):
    """make_float_vocabulary with every component rounded to a multiple of 1/64 (differences and mirrors stay exact)."""
    voc = bow_synth.make_float_vocabulary(k=k, L=L, dims=dims, seed=seed, **kw)
    voc["desc"] = (np.round(voc["desc"] * 64) / 64).astype(np.float32)
    return voc


@_register(CLASSES, "float_ties")
def float_ties():
    """Equal squared-L2 distances by construction: a later child is an earlier one mirrored about the feature in one
    component, so both sums add the same float32 terms in the same order."""
    rng = np.random.default_rng(401)
    k, L, dims = 4, 3, 16
    voc = _dyadic_float_voc(k, L, dims, 401, stop_frac=0.0)
    lv = _level_ranges(k, L)
    steps = {}
    for p in range(lv[L][0]):  # every internal node: child j = child i moved by 2 * step in component e
        i, j = [(0, 2), (1, 3), (0, 3), (2, 3)][p % 4]
        e, step = int(rng.integers(0, dims)), np.float32(rng.integers(1, 9)) / np.float32(64)
        voc["desc"][p * k + 1 + j] = voc["desc"][p * k + 1 + i]
        voc["desc"][p * k + 1 + j, e] += 2 * step
        steps[p] = (i, e, step)
    out = []
    for _ in range(400):
        p = int(rng.integers(0, lv[L][0]))
        i, e, step = steps[p]
        f = voc["desc"][p * k + 1 + i].copy()
        f[e] += step
        out.append(f)
    desc = np.concatenate([np.stack(out), bow_synth.float_features_near_words(voc, 100, seed=402)])
    return voc, desc, (0, 1), {"ties": (0.20, 0.05, 0.05)}


@_register(CLASSES, "float_nonfinite")
def float_nonfinite():
    """NaN, +-inf and FLT_MAX-scale features: no child compares below FLT_MAX and the descent stops at the root (weight 0:
    not in the BoW vector).  Node 2's children sit at 3e38 in one component, so every finite feature that reaches node 2
    stops there, on an internal node whose weight is positive.  The reference does not terminate on these."""
    rng = np.random.default_rng(501)
    k, L, dims = 3, 3, 8
    voc = _dyadic_float_voc(k, L, dims, 501, stop_frac=0.0)
    voc["desc"][2 * k + 1:2 * k + 1 + k, 3] = np.float32(3e38)
    voc["nodes"]["weight"][2] = np.float32(1.75)
    base = bow_synth.float_features_near_words(voc, 120, seed=502)
    bad = base[:60].copy()
    for r in range(60):
        e = int(rng.integers(0, dims))
        bad[r, e] = [np.nan, np.inf, -np.inf, 3.0e38, -3.4e38, 1.5e19][r % 6]
    bad[5::6, :] = np.float32(1.5e19)  # each square is finite (2.25e38); the running sum overflows at the second
    near2 = (voc["desc"][2] + rng.normal(size=(40, dims)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    desc = np.concatenate([bad, base[60:], near2]).astype(np.float32)
    return voc, desc, (0, 1, 2), {"stops_at": (0, 2), "reference": False}


def _one_word(n, flip):
    """Both sizes share one vocabulary (they ride in one batched call).  DOT scoring does not normalise, so the value is the
    n - 1 float adds themselves (divided by the vector size, 1)."""
    voc = bow_synth.make_vocabulary(k=4, L=3, seed=601, ragged=False, stop_frac=0.0, weighting=TF_IDF, scoring=DOT)
    leaf = int(np.random.default_rng(601).integers(_level_ranges(4, 3)[3][0], len(voc["nodes"])))
    voc["nodes"]["weight"][leaf] = np.float32(3.7)  # not a dyadic value: n - 1 float adds are not n * w
    desc = _near(voc, np.full(n, leaf), np.random.default_rng(600 + n), flip)
    return voc, desc, (1,), {"nb": 1}


_register(CLASSES, "one_word_16384")(functools.partial(_one_word, 16384, 0))  # 16384 copies: 64 sort slots per thread
_register(CLASSES, "one_word_257")(functools.partial(_one_word, 257, 1))      # one bit off each: P = 512


@_register(CLASSES, "all_stopped")
def all_stopped():
    voc = bow_synth.make_vocabulary(k=4, L=3, seed=701, scoring=L1)
    voc["nodes"]["weight"][:] = 0.0
    desc = bow_synth.features_near_words(voc, 300, seed=702)
    return voc, desc, (0, 2), {"nb": 0}


@_register(CLASSES, "all_distinct_pow2")
def all_distinct_pow2():
    """256 features, each exactly one of the 256 leaf descriptors, shuffled: nb == cap == P."""
    voc = bow_synth.make_vocabulary(k=4, L=4, seed=801, ragged=False, stop_frac=0.0, weighting=TF, scoring=L2)
    rng = np.random.default_rng(801)
    lo, hi = _level_ranges(4, 4)[4]
    desc = voc["desc"][rng.permutation(np.arange(lo, hi))].copy()
    return voc, desc, (0, 3), {"nb": 256}


@_register(CLASSES, "chain")
def chain():
    """childNum == 1 throughout: 0 -> 1 -> 3 -> 7 -> 15 -> 31."""
    rng = np.random.default_rng(901)
    k, L = 2, 5
    child_num = np.zeros(32, np.uint32)
    child_num[[0, 1, 3, 7, 15]] = 1
    weight = np.zeros(32, np.float32)
    weight[31] = 2.25
    voc = _hand_voc(k, L, child_num, weight, rng.integers(0, 256, (32, 32), dtype=np.uint8), weighting=TF, scoring=L1)
    return voc, rng.integers(0, 256, (70, 32), dtype=np.uint8), (0, 1, 2, 5, 8), {"nb": 1}


@_register(CLASSES, "root_only")
def root_only():
    rng = np.random.default_rng(1001)
    voc = _hand_voc(2, 1, np.zeros(1, np.uint32), np.array([1.5], np.float32), rng.integers(0, 256, (1, 32), dtype=np.uint8),
                    weighting=TF_IDF, scoring=DOT)
    return voc, rng.integers(0, 256, (33, 32), dtype=np.uint8), (0, 1, 2), {"nb": 1}


@_register(CLASSES, "k2_deep")
def k2_deep():
    voc = bow_synth.make_vocabulary(k=2, L=12, seed=1101, scoring=CHI2)
    desc = np.concatenate([bow_synth.features_near_words(voc, 400, seed=1102),
                           np.random.default_rng(1103).integers(0, 256, (100, 32), dtype=np.uint8)])
    return voc, desc, (0, 2, 11, 13), {}


def _bytes_edge(desc_bytes, k, L, n, seed):
    voc = bow_synth.make_vocabulary(k=k, L=L, seed=seed, desc_bytes=desc_bytes, stop_frac=0.0)
    desc = np.concatenate([bow_synth.features_near_words(voc, n - n // 3, seed=seed + 1, flip_bits=min(10, desc_bytes // 3 + 1)),
                           np.random.default_rng(seed + 2).integers(0, 256, (n // 3, desc_bytes), dtype=np.uint8)])
    return voc, desc, (0, 1), {}


_register(CLASSES, "narrow_wide_bytes_8")(functools.partial(_bytes_edge, 8, 4, 3, 200, 1201))
_register(CLASSES, "narrow_wide_bytes_16")(functools.partial(_bytes_edge, 16, 4, 3, 200, 1204))
_register(CLASSES, "narrow_wide_bytes_16384")(functools.partial(_bytes_edge, 16384, 2, 1, 3, 1207))  # ~ 100 KB in all


def _dims_edge(dims, k, L, n, seed):
    voc = bow_synth.make_float_vocabulary(k=k, L=L, dims=dims, seed=seed, stop_frac=0.0)
    return voc, bow_synth.float_features_near_words(voc, n, seed=seed + 1, sigma=0.3), (0, 1), {}


_register(CLASSES, "float_dims_edges_8")(functools.partial(_dims_edge, 8, 3, 2, 100, 1301))
_register(CLASSES, "float_dims_edges_4096")(functools.partial(_dims_edge, 4096, 2, 1, 4, 1304))


def _weighting_scoring(weighting, scoring):
    """600 features on a 64-leaf tree with a few stopped words: every word repeats many times."""
    voc = bow_synth.make_vocabulary(k=4, L=3, seed=1401, ragged=False, stop_frac=0.15, weighting=weighting, scoring=scoring)
    return voc, bow_synth.features_near_words(voc, 600, seed=1402, flip_bits=12), (0, 1), {"repeats": 10}


for _wt in (TF_IDF, TF, IDF, BINARY):
    for _sc in (L1, L2, DOT):
        _register(CLASSES, f"weighting_{_wt}_scoring_{_sc}")(functools.partial(_weighting_scoring, _wt, _sc))


def case(name):
    return CLASSES[name]()


def voc_key(voc):
    """Two classes with the same key can ride in one batched call."""
    return (voc["k"], voc["L"], voc["weighting"], voc["scoring"], voc["nodes"].tobytes(), voc["desc"].tobytes())


# ------------------------------------------------------------------------------------------------------ scoring classes
def _pad(vectors, cap, counts=None):
    ids = np.full((len(vectors), cap), NONE, np.uint32)
    vals = np.zeros((len(vectors), cap), np.float32)
    for r, (i, v) in enumerate(vectors):
        ids[r, :len(i)] = i
        vals[r, :len(i)] = v
    n = np.array([len(i) for i, _ in vectors] if counts is None else counts, np.int32)
    return ids, vals, n


def _vec(rng, ids):
    ids = np.asarray(ids, np.uint32)
    return ids, (rng.random(len(ids)).astype(np.float32) + np.float32(0.05)) / np.float32(max(len(ids), 1))


def _draw(rng, n, universe):
    return np.sort(rng.choice(universe, n, replace=False)).astype(np.uint32)


def _lengths(scoring):
    """Lengths 0 / 1 / 63 / 64 / 65 / 128 / 129 on both sides (the 64-lane ballot rounds), ids from a universe of 260."""
    rng = np.random.default_rng(2000 + scoring)
    lens = (0, 1, 63, 64, 65, 128, 129)
    qs = [_vec(rng, _draw(rng, n, 260)) for n in lens]
    ds = [_vec(rng, _draw(rng, n, 260)) for n in lens]
    return scoring, _pad(qs, 130), _pad(ds, 129), {"q_len": lens, "db_len": lens}


def _overlaps(scoring):
    """One 100-word query (ids 1000, 1010, ...) against: disjoint ids, itself, one common word first / in the middle / last,
    a database vector exhausted before the query, one that outlasts it, an empty one; then the empty query."""
    rng = np.random.default_rng(2100 + scoring)
    a = 1000 + 10 * np.arange(100)
    q = _vec(rng, a)
    other = lambda m: 5 + 10 * np.arange(m)  # never in a
    ds = [_vec(rng, other(70)), (q[0].copy(), q[1].copy()),
          _vec(rng, np.sort(np.r_[a[0], 2005 + 10 * np.arange(30)])),
          _vec(rng, np.sort(np.r_[a[50], 5 + 10 * np.arange(20), 2005 + 10 * np.arange(20)])),
          _vec(rng, np.sort(np.r_[a[99], 5 + 10 * np.arange(40)])),
          _vec(rng, np.r_[a[:30]]),                       # exhausted first: 70 query words in the tail loop
          _vec(rng, np.r_[a[60:], 5000 + np.arange(65)]),  # outlasts the query: 60 unmatched words inside the loop
          _vec(rng, [])]
    common = [[0, 100, 1, 1, 1, 30, 40, 0], [0] * 8]
    return scoring, _pad([q, _vec(rng, [])], 100), _pad(ds, 128), {"q_len": (100, 0), "db_len": (70, 100, 31, 41, 41, 30, 105, 0),
                                                                  "common": common}


def _zeros(scoring):
    """Zero values: common words with vi == 0, wi == 0 and both (vi + wi == 0), and unmatched zero-valued query words both
    while the database vector still has larger ids and after it is exhausted."""
    rng = np.random.default_rng(2200 + scoring)
    ids = 10 * np.arange(80)
    qi, qv = _vec(rng, ids)
    qv = qv.copy()
    qv[[3, 10, 11, 40, 70, 79]] = 0.0
    dbs = []
    di, dv = _vec(rng, ids[:60])  # exhausted before the query: query words 60.. (two of them zero) are in the tail
    dv = dv.copy()
    dv[[3, 5, 11, 41]] = 0.0      # word 3 and 11: both zero; 5 and 41: only the database side
    dbs.append((di, dv))
    keep = np.r_[np.arange(0, 8), np.arange(12, 80)]  # words 10, 11 (zero in the query) unmatched with larger ids remaining
    di, dv = _vec(rng, ids[keep])
    dv = dv.copy()
    dv[[0, 3]] = 0.0
    dbs.append((di, dv))
    dbs.append((qi.copy(), np.zeros_like(qv)))  # every value zero
    return scoring, _pad([(qi, qv)], 80), _pad(dbs, 80), {"q_len": (80,), "db_len": (60, 76, 80), "common": [[60, 76, 80]],
                                                          "zeros": True}


def _counts_over_cap(scoring):
    """counts above the capacity on both sides: the kernel must clamp to cap."""
    rng = np.random.default_rng(2300 + scoring)
    qs = [_vec(rng, _draw(rng, 64, 150)), _vec(rng, _draw(rng, 64, 150))]
    ds = [_vec(rng, _draw(rng, 70, 150)), _vec(rng, _draw(rng, 70, 150)), _vec(rng, _draw(rng, 9, 150))]
    return scoring, _pad(qs, 64, counts=[64 + 5, 64]), _pad(ds, 70, counts=[70 + 1, 1 << 30, 9]), {"q_len": (64, 64),
                                                                                                   "db_len": (70, 70, 9)}


def _ndb(n_db, scoring):
    rng = np.random.default_rng(2400 + 10 * n_db + scoring)
    qs = [_vec(rng, _draw(rng, n, 400)) for n in (200, 37)]
    ds = [_vec(rng, _draw(rng, int(rng.integers(1, 300)), 400)) for _ in range(n_db)]
    return scoring, _pad(qs, 200), _pad(ds, 300), {"q_len": (200, 37), "n_db": n_db}


def _cap_q(cap_q, scoring):
    """One full-length query: 16384 words are staged in 128 KB of LDS, 16385 search global memory, ~8000 take more than the
    default 48 KB of dynamic LDS."""
    rng = np.random.default_rng(2500 + cap_q % 1000 + scoring)
    q = _vec(rng, _draw(rng, cap_q, 60000))
    ds = [_vec(rng, _draw(rng, 3000, 60000)), (q[0].copy(), q[1].copy()), _vec(rng, q[0][:cap_q // 2:3]),
          _vec(rng, np.r_[q[0][cap_q // 2:], 70000 + np.arange(10)]), _vec(rng, [])]
    return scoring, _pad([q], cap_q), _pad(ds, cap_q), {"q_len": (cap_q,), "n_db": 5}


@_register(SCORE_CLASSES, "nq_65537")
def nq_65537():
    """65537 four-word queries against 5 vectors: the second launch of the n_q loop writes its rows past 65535 * n_db."""
    rng = np.random.default_rng(2600)
    n_q = 65537
    ids = rng.integers(0, 4, (n_q, 4)).astype(np.uint32) + np.arange(4, dtype=np.uint32)[None, :] * 4  # slot j: an id of 4j .. 4j+3
    vals = (rng.random((n_q, 4)).astype(np.float32) + np.float32(0.05)) / np.float32(4)
    n = rng.integers(0, 5, n_q).astype(np.int32)
    n[[0, 65534, 65535, 65536]] = 4
    ds = [_vec(rng, rng.integers(0, 4, 4) + np.arange(4) * 4) for _ in range(4)] + [_vec(rng, [0, 5, 10, 15])]
    return L1, (ids, vals, n), _pad(ds, 4), {"n_q": n_q, "n_db": 5}


for _sc in range(6):
    _register(SCORE_CLASSES, f"lengths_s{_sc}")(functools.partial(_lengths, _sc))
    _register(SCORE_CLASSES, f"overlaps_s{_sc}")(functools.partial(_overlaps, _sc))
    _register(SCORE_CLASSES, f"zeros_s{_sc}")(functools.partial(_zeros, _sc))
    _register(SCORE_CLASSES, f"counts_over_cap_s{_sc}")(functools.partial(_counts_over_cap, _sc))
for _sc in (L1, KL):
    for _n in (1, 3, 5):
        _register(SCORE_CLASSES, f"ndb_{_n}_s{_sc}")(functools.partial(_ndb, _n, _sc))
    for _c in (16384, 16385, 8000):
        _register(SCORE_CLASSES, f"capq_{_c}_s{_sc}")(functools.partial(_cap_q, _c, _sc))


def score_case(name):
    return SCORE_CLASSES[name]()


def random_tree(rng, k, L, leaf_frac, stop_frac, weighting, scoring, width, is_float):
    """A random tree for the fuzz: 1..k children per internal node, early leaves on levels 1..L-1 with probability
    leaf_frac, stopped words with probability stop_frac; width = descriptor bytes, or float dimensions."""
    lv = _level_ranges(k, L)
    nnodes = lv[L][1]
    child_num = np.zeros(nnodes, np.uint32)
    child_num[:lv[L][0]] = np.where(rng.random(lv[L][0]) < 0.5, k, rng.integers(1, k + 1, lv[L][0]))
    early = np.arange(lv[1][0], lv[L][0])
    child_num[early[rng.random(len(early)) < leaf_frac]] = 0
    weight = np.where(child_num == 0, rng.uniform(0.5, 9.0, nnodes), 0.0).astype(np.float32)
    weight[(child_num == 0) & (rng.random(nnodes) < stop_frac)] = 0.0
    parent = np.maximum((np.arange(nnodes) - 1) // k, 0)
    if is_float:
        desc = (rng.integers(-64, 65, (nnodes, width)) / 16.0).astype(np.float32)  # a coarse grid: exact ties do occur
        for lo, hi in lv[1:]:
            desc[lo:hi] = desc[parent[lo:hi]] + desc[lo:hi] / np.float32(4)
    else:
        desc = rng.integers(0, 256, (nnodes, width), dtype=np.uint8)
        for lo, hi in lv[1:]:
            desc[lo:hi] = desc[parent[lo:hi]] ^ (desc[lo:hi] & rng.integers(0, 256, (hi - lo, width), dtype=np.uint8)
                                                 & rng.integers(0, 256, (hi - lo, width), dtype=np.uint8))
    return _hand_voc(k, L, child_num, weight, desc, weighting=weighting, scoring=scoring)


def random_features(rng, voc, n):
    """Half near (or exactly on) a random node's descriptor, half unrelated."""
    d = voc["desc"][rng.integers(0, len(voc["nodes"]), n)].copy()
    if d.dtype == np.float32:
        d += (rng.integers(-2, 3, d.shape) / 16.0).astype(np.float32)
        far = (rng.integers(-80, 81, d.shape) / 16.0).astype(np.float32)
    else:
        d ^= (rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8)
              & rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8))
        far = rng.integers(0, 256, d.shape, dtype=np.uint8)
    pick = rng.random(n) < 0.5
    d[pick] = far[pick]
    return d


def score_voc(scoring):
    """A three-node vocabulary whose scoring object is `scoring` (what a reference Vocabulary needs to score at all)."""
    rng = np.random.default_rng(77)
    return _hand_voc(2, 1, np.array([2, 0, 0], np.uint32), np.array([0, 1, 2], np.float32),
                     rng.integers(0, 256, (3, 32), dtype=np.uint8), scoring=scoring)
