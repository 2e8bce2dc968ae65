"""Inputs of the two-view tests (tests/test_two_view_cpu.py takes their census with the restatement, tests/test_two_view_gpu.py
runs them on the device): one batch for gh_two_view_batch_dev and three synthetic frames for gh_two_view_pairs_dev.  numpy
is used to GENERATE inputs only; expected results come from two_view_restate."""
import functools

import numpy as np

import two_view_restate as tv

# the census batch is evaluated with these (the defaults would call the small 10 + 7 / 10 + 8 mixes TOO_FEW)
BATCH_PARAMS = dict(min_parallax_cos=0.99998, max_reproj=0.004, min_good=8, min_good_permille=500)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)  # the wave and workgroup boundaries of the row loop
FILL_POINT, FILL_GOOD = 7.0, 0xAB


def rot(axis, angle):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


R_TRUE, T_TRUE = rot([0.2, 1.0, 0.1], 0.12), np.array([0.6, 0.05, 0.1])  # the two views of tests/test_ransac_oracle.py


def essential(R, t):
    """[t]x R: dst^T E src = 0 for X_cur = R X_ref + t."""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return (tx @ R).reshape(9)


def scene(n, seed, R=R_TRUE, t=T_TRUE, noise=0.0, far=1.0):
    """n points in front of both views -> (src n x 2, dst n x 2, X n x 3), normalised coordinates, X_cur = R X_ref + t."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-3, 3, (n, 2)), rng.uniform(4, 9, n)] * far
    X2 = X @ R.T + t
    assert (X2[:, 2] > 0).all()
    p2 = X2[:, :2] / X2[:, 2:3] + rng.normal(size=(n, 2)) * noise
    return X[:, :2] / X[:, 2:3], p2, X


def _problem(name, E, src, dst, mask=None):
    return dict(name=name, E=np.asarray(E, np.float64).reshape(9), src=np.asarray(src, np.float64).reshape(-1, 2),
                dst=np.asarray(dst, np.float64).reshape(-1, 2), mask=None if mask is None else np.asarray(mask, np.uint8))


def _mix(name, n_plus, n_minus, seed):
    """Rows generated under (R, +t) and under (R, -t) for ONE E: two candidates collect n_plus and n_minus rows."""
    s1, d1, _ = scene(n_plus, seed)
    s2, d2, _ = scene(n_minus, seed + 1, t=-T_TRUE)
    return _problem(name, essential(R_TRUE, T_TRUE), np.r_[s1, s2], np.r_[d1, d2])


@functools.lru_cache(maxsize=None)
def batch_problems():
    """The problems of the census batch, in batch order.  Empty ones sit first, in the middle and last."""
    E = essential(R_TRUE, T_TRUE)
    empty = lambda name: _problem(name, E, np.zeros((0, 2)), np.zeros((0, 2)))
    probs = [empty("empty_first")]
    # {E, -E} x {t, -t} over the row counts: the four candidate indices win
    for k, n in enumerate(ROW_COUNTS):
        t = T_TRUE if k % 2 == 0 else -T_TRUE
        s, d, _ = scene(n, 100 + k, t=t)
        probs.append(_problem("rows_%d" % n, essential(R_TRUE, t) * (1.0 if (k // 2) % 2 == 0 else -1.0), s, d))
    s, d, _ = scene(20, 7)
    probs.append(_problem("zero_E", np.zeros(9), s, d))
    nanE = E.copy()
    nanE[4] = np.nan
    probs.append(_problem("nan_E", nanE, s, d))
    probs.append(_problem("rank1_E", np.outer([1.0, 2.0, -0.5], [0.3, -1.0, 2.0]).reshape(9), s, d))
    s, d, _ = scene(200, 8, far=1000.0)
    probs.append(_problem("far_scene", E, s, d))
    probs.append(empty("empty_middle"))
    probs.append(_mix("mix_10_7", 10, 7, 20))
    probs.append(_mix("mix_10_8", 10, 8, 30))
    probs.append(_mix("mix_50_50", 50, 50, 40))
    # 30 true rows among 70 rows that belong to nothing: enough good rows, too small a share
    rng = np.random.default_rng(9)
    s, d, _ = scene(100, 50)
    d[30:] = rng.uniform(-0.6, 0.6, (70, 2))
    probs.append(_problem("low_share", E, s, d))
    # a mask with holes, an all-zero mask
    s, d, _ = scene(257, 60)
    holes = (rng.random(257) < 0.7).astype(np.uint8)
    holes[[0, 63, 64, 255, 256]] = (0, 1, 0, 1, 0)
    probs.append(_problem("mask_holes", E, s, d, holes * 3))  # (any non-zero byte takes part)
    probs.append(_problem("mask_zero", E, s, d, np.zeros(257, np.uint8)))
    # NaN / Inf rows, wrong matches and rays that are exactly parallel under the true rotation inside a good problem
    s, d, _ = scene(300, 70, noise=0.0005)
    s[3], d[17, 1], s[64, 0], d[200] = np.nan, np.nan, np.inf, (-np.inf, 0.1)
    d[100:130] += rng.uniform(0.05, 0.3, (30, 2)) * rng.choice([-1, 1], (30, 2))
    a = np.c_[s[250:260], np.ones(10)] @ R_TRUE.T
    d[250:260] = a[:, :2] / a[:, 2:3]
    probs.append(_problem("dirty_rows", E, s, d))
    # an estimate that is not exactly essential is decomposed all the same
    s, d, _ = scene(120, 80)
    probs.append(_problem("not_essential", E + 1e-3 * rng.normal(size=9), s, d))
    probs.append(empty("empty_last"))
    return tuple(probs)


@functools.lru_cache(maxsize=None)
def batch_arrays(e_stride):
    """-> dict(E flat nproblems x e_stride, src, dst, mask rows, offsets nproblems + 1 + the odd ranges, names).  After the
    census problems come three more E rows whose ranges are reversed, outside the arrays and negative; the rows between
    the last regular problem and offsets[-1] belong to nobody.  The reversed range makes the range after it overlap the
    last regular rows: that problem has an all-zero E and the rows it shares are masked out, so both write zeros."""
    probs = list(batch_problems())
    s, d, _ = scene(40, 90)
    m = np.ones(40, np.uint8)
    m[30:] = 0
    probs.append(_problem("before_reversed", essential(R_TRUE, T_TRUE), s, d, m))
    src = np.concatenate([p["src"] for p in probs])
    dst = np.concatenate([p["dst"] for p in probs])
    mask = np.concatenate([np.ones(len(p["src"]), np.uint8) if p["mask"] is None else p["mask"] for p in probs])
    off = np.zeros(len(probs) + 1, np.int64)
    off[1:] = np.cumsum([len(p["src"]) for p in probs])
    total = int(off[-1])
    pad = 16  # rows nobody owns
    src = np.r_[src, np.full((pad, 2), 0.25)]
    dst = np.r_[dst, np.full((pad, 2), 0.25)]
    mask = np.r_[mask, np.ones(pad, np.uint8)]
    # offsets: ... total | total - 10 (reversed) | total (overlaps the masked tail, zero E) | 10**6 (outside) | -5 (outside,
    # then negative begin) | total + pad (negative begin) ; the last entry is the limit
    extra = [total - 10, total, 10 ** 6, -5, total + pad]
    names = [p["name"] for p in probs] + ["reversed", "overlap_zero_E", "past_the_end", "from_past_the_end", "negative_begin"]
    off = np.r_[off, extra].astype(np.int32)
    Es = [p["E"] for p in probs] + [essential(R_TRUE, T_TRUE), np.zeros(9)] + [essential(R_TRUE, T_TRUE)] * 3
    E = np.full((len(Es), e_stride), 123.0)
    E[:, :9] = np.asarray(Es)
    assert len(names) == len(off) - 1 == len(Es)
    return dict(E=E.reshape(-1), src=src, dst=dst, mask=mask, offsets=off, names=names, e_stride=e_stride)


@functools.lru_cache(maxsize=None)
def batch_expected():
    """The restatement's result for batch_arrays (the same for every e_stride), computed once and shared."""
    a = batch_arrays(9)
    return tv.two_view_batch(a["E"].tolist(), 9, a["src"].tolist(), a["dst"].tolist(), a["offsets"].tolist(),
                             a["mask"].tolist(), fill_point=FILL_POINT, fill_good=FILL_GOOD, **BATCH_PARAMS)


# ---------------------------------------------------------------- the pair entry
CAP = 320
COUNTS = (320, 300, 0)                        # one frame is full, one is empty
PAIRS = ((0, 1), (1, 0), (0, 2), (2, 2))      # the true pair, its reverse, an empty train frame, an empty query frame
FX, FY, CX, CY = 500.0, 510.0, 320.0, 240.0
PAIR_THR = 1e-7    # threshold of the essential fit, normalised units: near the noise, so the inlier count ranks the samples
PAIR_SEED = 3
# Two verging views, baseline / depth about 0.5: the winner of a RANSAC is a MINIMAL 8-point estimate and multiplies the
# noise of its sample; this geometry keeps the factor small.
R_PAIR, T_PAIR = rot([0.2, 1.0, 0.1], -0.3), np.array([2.5, 0.2, 1.0])
# Noise of the pair test: none is added.  The keypoint records are float32 PIXELS, so every coordinate carries the rounding of
# its record: at most 2^-15 px (half an ulp below 1024 px) = 6e-8 in normalised units at f = 500.  tests/test_two_view_cpu.py
# checks with the oracle's fit and the restatement that the pose then comes back to 1e-6 (measured: 4e-7 at the worst over
# eight seeds and both directions of the pair).


@functools.lru_cache(maxsize=None)
def pair_frames():
    """Three frames of keypoint records projected from one scene and the match rows of PAIRS, built by hand: 25 % wrong
    matches, -1 entries, a keep mask with holes.  Rows past a frame's count hold coordinates nobody may read."""
    from gslam_amd.orb import KP_DTYPE
    rng = np.random.default_rng(2025)
    X = np.c_[np.random.default_rng(11).uniform(-3, 3, (CAP, 2)), np.random.default_rng(12).uniform(3, 7, CAP)]
    X2 = X @ R_PAIR.T + T_PAIR
    assert (X2[:, 2] > 0).all()
    p1, p2 = X[:, :2] / X[:, 2:3], X2[:, :2] / X2[:, 2:3]
    kps = np.zeros((3, CAP), KP_DTYPE)
    kps["x"], kps["y"] = 1e9, -1e9
    kps["size"], kps["octave"], kps["class_id"] = 31.0, 0, -1
    perm = rng.permutation(CAP)               # frame 1 row r shows point perm[r]; its count cuts the last 20 off
    where = np.argsort(perm)                  # point i is row where[i] of frame 1
    kps["x"][0], kps["y"][0] = FX * p1[:, 0] + CX, FY * p1[:, 1] + CY
    kps["x"][1], kps["y"][1] = FX * p2[perm, 0] + CX, FY * p2[perm, 1] + CY
    idx1 = np.full((len(PAIRS), CAP), -1, np.int32)
    idx1[0] = where
    idx1[1] = perm
    idx1[2] = rng.integers(0, CAP, CAP)
    idx1[3] = np.arange(CAP)
    for p in (0, 1):
        wrong = rng.random(CAP) < 0.25
        idx1[p, wrong] = rng.integers(0, CAP, int(wrong.sum()))
        idx1[p, rng.choice(CAP, 8, replace=False)] = -1
        idx1[p, rng.choice(CAP, 4, replace=False)] = (CAP, 65535, 2 ** 31 - 1, -7)
    keep = (rng.random((len(PAIRS), CAP)) < 0.9).astype(np.uint8)
    return kps, np.array(COUNTS, np.int32), idx1, keep


def normalise(xy):
    """Pixels (float64 of the float32 records) -> normalised coordinates, the pair entry's rule in numpy float64."""
    out = np.empty_like(xy)
    out[:, 0] = (xy[:, 0] - CX) / FX
    out[:, 1] = (xy[:, 1] - CY) / FY
    return out
