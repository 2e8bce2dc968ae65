"""Adversarial correspondences for the estimator parity tests (gh_ransac_estimate_ex vs oracle/ransac_oracle.c, and the
oracle vs the independent numpy restatement).  Every builder is seeded and pure numpy; no GPU, no oracle.

CLASSES maps a class name to builder(model, seed) -> (src, dst, threshold, expect), or None where the class does not
apply to the model.  `expect` names the branch the class is built to reach; tests/test_ransac_adversarial_oracle.py
holds every class to it (the census) before a GPU sees the data.  It is one name for all three sampling modes or a
3-tuple (RANSAC, LMEDS, NOSAMPLE):

  "model"       a model with at least s inliers comes back
  "no_model"    count 0, model all zero, mask all zero
  "ties"        at least two hypotheses share the maximal count (RANSAC) / the minimal median (LMedS)
  "all_inliers" every row fits every valid hypothesis: the confidence rule stops at the first valid one
  "median_inf"  LMedS: every hypothesis has more than half of its errors undefined -> no model
  "projection"  model 4: the winner scores inliers as a fundamental matrix and its essential projection fails -> no model
  "any"         valid but ambiguous or ill-conditioned input: only parity and count == popcount(mask) are asked

The nominal data come from tests/test_ransac_oracle.py (_corr, _two_view, _all_model_cases)."""
import functools

import numpy as np

from test_ransac_oracle import _all_model_cases, _corr, _two_view

RANSAC, LMEDS, NOSAMPLE = 0, 1, 2
MODELS = tuple(range(8))
S_OF = (4, 3, 8, 4, 8, 3, 3, 6)        # minimal sample
MS_OF = (9, 6, 9, 12, 9, 8, 4, 12)     # model doubles
DIM_P = (2, 2, 2, 3, 2, 3, 3, 3)
DIM_Q = (2, 2, 2, 3, 2, 3, 3, 2)
THR = (2.0, 2.0, 1.0, 0.05, 0.002, 0.02, 0.01, 0.003)
_NOISE = {0: 0.3, 1: 0.3, 2: 0.2, 3: 0.005}
SEEDS = (0, 1, 2 ** 63, 2 ** 64 - 1)   # estimator seeds every parity test runs the nominal class under

# The large class.  One oracle call (2048 hypotheses x n errors, LMedS sorts each), measured on an idle x86 build machine,
# one thread, A2 / plane (the two cheapest errors):
#   RANSAC   n = 65 537: 0.42 / 0.40 s   100 003: 0.71 / 0.58 s   200 003: 1.29 / 1.10 s   -> 200 003 (A2)
#   LMedS    n = 65 537: 18.7 / 14.5 s   100 003: 25.4 / 20.9 s   200 003: 55.8 / 39.6 s
# No LMedS candidate stays under 10 s (qsort of n doubles, 2048 times); the smallest one is kept, on the plane, so that the
# radix select still sees more than 65 536 keys once.
LARGE_N = {RANSAC: 200003, LMEDS: 65537, NOSAMPLE: 200003}
LARGE_MODEL = {RANSAC: 1, LMEDS: 6, NOSAMPLE: 1}


def expect_for(expect, sampling):
    return expect if isinstance(expect, str) else expect[sampling]


@functools.lru_cache(maxsize=None)
def _base():
    return {c[0]: c[1:] for c in _all_model_cases()}


def nominal(model, n, seed=0):
    """n correspondences of the well-conditioned case of tests/test_ransac_oracle.py, 25-30 % outliers."""
    if model in (0, 1, 2, 3):
        P, Q, _, _ = _corr(model, n, 0.28, 40 + model + seed, _NOISE[model])
    elif model == 4:
        P, Q, _, _ = _two_view(n, 0.25, 33 + seed, 0.0005)
    else:  # the 600 rows of _all_model_cases, cycled (rows repeat beyond 600)
        P, Q, _, _ = _base()[model]
        idx = (np.arange(n) + 7 * seed) % len(P)
        P, Q = P[idx], Q[idx]
    return np.ascontiguousarray(P, dtype=np.float64).copy(), np.ascontiguousarray(Q, dtype=np.float64).copy(), THR[model]


def _rng(model, seed, salt):
    return np.random.default_rng([salt, model, seed])


CLASSES = {}


def _register(name):
    def deco(f):
        CLASSES[name] = f
        return f
    return deco


# ---------------------------------------------------------------- nominal and sizes
@_register("nominal")
def _nominal(model, seed):
    P, Q, thr = nominal(model, 300, seed)
    return P, Q, thr, ("model", "model", "any")


def _sized(n_of, expect):
    def build(model, seed):
        n = n_of(model)
        P, Q, thr = nominal(model, n, seed)
        return P, Q, thr, expect(model, n) if callable(expect) else expect
    return build


# n = s - 1: below the sample, the entry's early exit.  n = s: the rejection sampler draws a full permutation and LMedS
# divides by max(n - s, 1).  With s or s + 1 rows, 28 % of them outliers, a model need not fit anything but its sample.
CLASSES["n_s_minus_1"] = _sized(lambda m: S_OF[m] - 1, "no_model")
for _k in (0, 1, 2):
    CLASSES["n_s_plus_%d" % _k] = _sized(lambda m, k=_k: S_OF[m] + k, "any")
# one workgroup of the scoring kernels strides by 256; the mask kernel has 256 rows per block; a wave is 64
for _n in (63, 64, 65, 255, 256, 257, 511, 513):
    CLASSES["block_%d" % _n] = _sized(lambda m, n=_n: n, ("model", "model", "any"))


def large(sampling, seed=0):
    """Past 65 536 rows: (model, src, dst, threshold, expect) of the size LARGE_N gives the sampling mode."""
    model = LARGE_MODEL[sampling]
    P, Q, thr = nominal(model, LARGE_N[sampling], seed)
    return model, P, Q, thr, ("model", "model", "any")[sampling]


# ---------------------------------------------------------------- coincident / collinear / coplanar
@_register("coincident")
def _coincident(model, seed):
    """All rows equal: every minimal sample is singular; only the eigenvector fits of NOSAMPLE (F, E, plane, PnP) and
    Horn's norms (exactly 0) are left to decide."""
    P, Q, thr = nominal(model, 50, seed)
    P[:], Q[:] = P[0], Q[0]
    return P, Q, thr, ("no_model", "no_model", "no_model" if model in (1, 3, 5) else "any")


@_register("collinear")
def _collinear(model, seed):
    """All sources on the x axis (exact zeros in the other coordinates).  H, A2, A3, plane, PnP: every sample is singular.
    F / E: columns uy, vy, y of the 8 x 9 system are zero, rank <= 6, the seventh pivot is an exact 0.
    SIM3: Horn's N has a double top eigenvalue, the rotation about the line is arbitrary but defined."""
    P, Q, thr = nominal(model, 120, seed)
    P[:, 1:] = 0.0
    if model == 6:
        Q = P.copy()
    if model == 5:
        return P, Q, thr, "any"
    # (E, NOSAMPLE: the zero y column is the "smallest eigenvector", F has rank 1 and the essential projection fails)
    return P, Q, thr, ("no_model", "no_model", "projection" if model == 4 else "any")


@_register("coplanar")
def _coplanar(model, seed):
    """A3 and PnP with every object point on Z = 0 (a zero column in the system: singular, exactly).  F / E on a planar
    scene with the nominal image noise: valid but ambiguous (without the noise the last pivots are rounding below 1e-12 and
    every sample is refused), the estimate is whatever the noise makes of the three-dimensional null space."""
    if model in (3, 7):
        P, Q, thr = nominal(model, 150, seed)
        P[:, 2] = 0.0
        return P, Q, thr, ("no_model", "no_model", "any")
    if model in (2, 4):
        rng = _rng(model, seed, 11)
        n = 200
        X = np.c_[rng.uniform(-3, 3, (n, 2)), np.full(n, 6.0)]
        X[:, 2] += 0.25 * X[:, 0]  # a slanted plane
        th = 0.1
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        X2 = X @ R.T + np.array([0.5, 0.05, 0.1])
        p1, p2 = X[:, :2] / X[:, 2:3], X2[:, :2] / X2[:, 2:3]
        if model == 2:
            p1, p2 = 500 * p1 + 320, 500 * p2 + 240
        p2 = p2 + rng.normal(size=p2.shape) * (0.2 if model == 2 else 0.0005)
        return p1, p2, THR[model], ("model", "model", "any")
    return None


@_register("pure_rotation")
def _pure_rotation(model, seed):
    """F / E with no baseline (and the nominal image noise): the epipolar constraint holds for a family of matrices."""
    if model not in (2, 4):
        return None
    rng = _rng(model, seed, 12)
    n = 200
    X = np.c_[rng.uniform(-3, 3, (n, 2)), rng.uniform(4, 9, n)]
    th = 0.1
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    X2 = X @ R.T
    p1, p2 = X[:, :2] / X[:, 2:3], X2[:, :2] / X2[:, 2:3]
    if model == 2:
        p1, p2 = 500 * p1 + 320, 500 * p2 + 240
    p2 = p2 + rng.normal(size=p2.shape) * (0.2 if model == 2 else 0.0005)
    return p1, p2, THR[model], ("model", "model", "any")


# ---------------------------------------------------------------- few distinct points
@_register("five_distinct")
def _five_distinct(model, seed):
    """Five distinct correspondences repeated to n = 300: a sample is regular only if its rows are distinct points, so
    nearly every one is singular (for s > 5, every one)."""
    P, Q, thr = nominal(model, 5, seed)
    idx = _rng(model, seed, 13).integers(0, 5, 300)
    return P[idx], Q[idx], thr, "any"


@_register("s_distinct_good")
def _s_distinct_good(model, seed):
    """s distinct noise-free inliers, each repeated, among distinct outliers: the few samples that draw s different good
    rows all give the same model."""
    s = S_OF[model]
    rng = _rng(model, seed, 14)
    P, Q, thr = nominal(model, 600, seed)
    inl = _inlier_flags(model, seed)
    good = np.flatnonzero(inl)[:s]
    bad = np.flatnonzero(~inl)[:40]
    idx = np.r_[rng.integers(0, s, 110), s + np.arange(40)]
    rng.shuffle(idx)
    rows = np.r_[good, bad][idx]
    return P[rows], Q[rows], thr, "any"


def _inlier_flags(model, seed):
    if model in (0, 1, 2, 3):
        return _corr(model, 600, 0.28, 40 + model + seed, _NOISE[model])[2]
    if model == 4:
        return _two_view(600, 0.25, 33 + seed, 0.0005)[2]
    inl = _base()[model][3]
    return inl[(np.arange(600) + 7 * seed) % len(inl)]


# ---------------------------------------------------------------- magnitudes
def _scaled(f):
    def build(model, seed):
        """The nominal case times f, both sides where the model is scale-covariant (H, A2, A3, SIM3, plane and the pixel
        coordinates of F), threshold alike.  E and PnP are tied to normalised image coordinates: PnP scales the object
        points only, E is left out.  At 1e-6 the absolute 1e-12 pivots reject samples the nominal case accepts."""
        if model == 4:
            return None
        P, Q, thr = nominal(model, 300, seed)
        if model == 7:
            return P * f, Q, thr, "any"
        return P * f, Q * f, thr * f, "any"
    return build


CLASSES["scale_1e4"] = _scaled(1e4)
CLASSES["scale_1e6"] = _scaled(1e6)
CLASSES["scale_1e-6"] = _scaled(1e-6)


# ---------------------------------------------------------------- non-finite coordinates
def _nonfinite(side, share):
    def build(model, seed):
        """NaN, +Inf and -Inf in a share of the rows.  F / E: the Hartley means are not finite and no row scores.  The
        others: hypotheses that draw a bad row carry NaN, the bad rows have undefined errors under every model."""
        rng = _rng(model, seed, 15)
        P, Q, thr = nominal(model, 300, seed)
        if model == 6:
            Q = P  # the plane reads src only
        rows = rng.choice(300, max(6, int(share * 300)), replace=False)
        vals = np.array([np.nan, np.inf, -np.inf])[np.arange(len(rows)) % 3]
        if side in ("src", "both"):
            P[rows, rng.integers(0, P.shape[1], len(rows))] = vals
        if side in ("dst", "both") and model != 6:
            Q[rows, rng.integers(0, Q.shape[1], len(rows))] = vals
        if model == 6:
            Q = P.copy()
        if model in (2, 4):  # (NOSAMPLE: the Jacobi fit never refuses; a fit that is not finite is no model)
            return P, Q, thr, "no_model"
        if share > 0.5:
            return P, Q, thr, ("any", "median_inf", "any")
        return P, Q, thr, ("model", "model", "any")
    return build


CLASSES["nonfinite_src"] = _nonfinite("src", 0.02)
CLASSES["nonfinite_dst"] = _nonfinite("dst", 0.02)
CLASSES["nonfinite_both"] = _nonfinite("both", 0.02)
CLASSES["nonfinite_fifth"] = _nonfinite("src", 0.2)      # the companion of the next one: a model still comes back
CLASSES["nonfinite_majority"] = _nonfinite("src", 0.55)  # LMedS: rank n / 2 is +inf under every hypothesis


# ---------------------------------------------------------------- exact arithmetic: ties
def _exact_data(model, seed, n, outlier_share, spread=3):
    """Integer correspondences on which solve and score are exact in binary64.  A2 / A3: sources on the corners of the
    unit square / cube (every regular sample has determinant +-1, so all pivots and multipliers are 0 or +-1), an integer
    model, outliers displaced by integers: every model and every squared error is an integer.  Plane: inliers on z = 0
    with integer x, y (normal (0, 0, +-1) exactly), outliers at integer heights."""
    rng = _rng(model, seed, 16)
    bad = rng.random(n) < outlier_share
    if model == 1:
        P = rng.integers(0, 2, (n, 2)).astype(np.float64)
        Q = P @ np.array([[2.0, -1.0], [1.0, 3.0]]).T + np.array([5.0, -7.0])
    elif model == 3:
        P = rng.integers(0, 2, (n, 3)).astype(np.float64)
        Q = P @ np.array([[2.0, -1.0, 0.0], [1.0, 3.0, -2.0], [0.0, 1.0, 1.0]]).T + np.array([5.0, -7.0, 2.0])
    elif model == 6:
        P = np.c_[rng.integers(-8, 9, (n, 2)), np.zeros(n)].astype(np.float64)
        P[bad, 2] = rng.integers(1, spread + 1, int(bad.sum())) * rng.choice([-1, 1], int(bad.sum()))
        return P, P.copy(), bad
    else:
        return None
    d = rng.integers(1, spread + 1, (int(bad.sum()), Q.shape[1])) * rng.choice([-1, 1], (int(bad.sum()), Q.shape[1]))
    Q[bad] += d
    return P, Q, bad


EXACT_MODELS = (1, 3, 6)


def _ties(thr, outlier_share, expect):
    def build(model, seed):
        d = _exact_data(model, seed, 301, outlier_share)
        if d is None:
            return None
        return d[0], d[1], thr, expect
    return build


CLASSES["ties_thr_0"] = _ties(0.0, 0.3, ("ties", "ties", "any"))
CLASSES["ties_thr_half"] = _ties(0.5, 0.3, ("ties", "ties", "any"))
CLASSES["ties_all_inliers"] = _ties(0.0, 0.0, ("all_inliers", "ties", "model"))


def _two_structures(thr):
    def build(model, seed):
        """Two equally supported exact structures, 152 rows each, every corner of the unit square / cube equally often in
        both: A2 / A3 with the integer model of _exact_data and the same model shifted by +1 in the first destination
        coordinate; the planes z = 0 and z = 1 over the same integer (x, y).  Hypotheses of either structure reach the same
        count (152) and, the errors of the other structure's rows being all 1, the same median (1.0) -- with DIFFERENT
        models, so which index wins a tie shows in the model that comes back.  Mixed samples give dyadic models too
        (determinant +-1 or +-2), still exact, which join the ties or (A3, threshold 0.5; LMedS) take the optimum over
        among themselves.  The plane has the class at threshold 0 only (at 0.5 one tilted plane wins alone)."""
        rng = _rng(model, seed, 20)
        if model in (1, 3):
            d = DIM_P[model]
            corners = np.array([[(c >> k) & 1 for k in range(d)] for c in range(2 ** d)], np.float64)
            per = 152 // len(corners)
            P = np.tile(np.repeat(corners, per, axis=0), (2, 1))
            M = np.array([[2.0, -1.0], [1.0, 3.0]]) if model == 1 else np.array([[2.0, -1.0, 0.0], [1.0, 3.0, -2.0], [0.0, 1.0, 1.0]])
            Q = P @ M.T + np.array([5.0, -7.0, 2.0])[:d]
            Q[152:, 0] += 1.0
        elif model == 6 and thr == 0.0:
            xy = rng.integers(-8, 9, (152, 2)).astype(np.float64)
            P = np.r_[np.c_[xy, np.zeros(152)], np.c_[xy, np.ones(152)]]
            Q = P.copy()
        else:
            return None
        perm = rng.permutation(304)
        # (plane: a tilted plane through both levels has the single smallest median, LMedS has no tie there)
        return P[perm], Q[perm], thr, ("ties", "any" if model == 6 else "ties", "any")
    return build


CLASSES["ties_two_structures_thr_0"] = _two_structures(0.0)
CLASSES["ties_two_structures_thr_half"] = _two_structures(0.5)


@_register("ties_int_general")
def _ties_int_general(model, seed):
    """H, A2, A3 on general integer coordinates with dyadic coefficients, outliers displaced by integers >= 8, threshold
    0.5: elimination rounds (pivots are not powers of two), but an all-inlier sample misses no inlier by more than 1e-9,
    so all of them reach the same count."""
    rng = _rng(model, seed, 17)
    n = 240
    bad = rng.random(n) < 0.3
    if model in (0, 1):
        P = rng.integers(0, 64, (n, 2)).astype(np.float64)
        Q = P @ np.array([[1.5, -0.25], [0.5, 1.25]]).T + np.array([4.0, -6.0])
    elif model == 3:
        P = rng.integers(0, 32, (n, 3)).astype(np.float64)
        Q = P @ np.array([[1.5, -0.25, 0.0], [0.5, 1.25, -0.5], [0.0, 0.75, 1.0]]).T + np.array([4.0, -6.0, 2.0])
    else:
        return None
    Q[bad] += rng.integers(8, 40, (int(bad.sum()), Q.shape[1])) * rng.choice([-1, 1], (int(bad.sum()), Q.shape[1]))
    return P, Q, 0.5, ("ties", "any", "any")


# ---------------------------------------------------------------- quantised errors for the median
def _quantised(n, exact_share, scale=1.0):
    def build(model, seed):
        """A2 / A3 on the exact corner data with every destination displaced by -1, 0 or +1 per coordinate: squared errors
        are small integers (times scale^2), so rank n / 2 of the radix select falls inside a long run of equal keys.
        exact_share of the rows are undisturbed: above one half the winning median is exactly 0, below it is scale^2 or
        2 scale^2.  scale = 2^-535 makes those medians denormal (2^-1070 = 16 ulp of the smallest denormal, still exact);
        the sources stay 0 / 1 so the pivots hold."""
        if model not in (1, 3):
            return None
        rng = _rng(model, seed, 18)
        P, Q, _ = _exact_data(model, seed, n, 0.0)
        Q = Q - np.array([5.0, -7.0, 2.0])[:Q.shape[1]]  # no offset: the scaled variant keeps every term denormal-safe
        move = rng.random(n) >= exact_share
        Q[move] += rng.integers(-1, 2, (int(move.sum()), Q.shape[1]))
        return P, Q * scale, 0.0, ("any", "ties", "any")
    return build


CLASSES["quantised_odd"] = _quantised(301, 0.35)
CLASSES["quantised_even"] = _quantised(300, 0.35)
CLASSES["quantised_median_zero"] = _quantised(301, 0.65)
CLASSES["quantised_denormal"] = _quantised(301, 0.35, scale=2.0 ** -535)


# ---------------------------------------------------------------- essential projection failure
@_register("projection_failure")
def _projection_failure(model, seed):
    """Model 4, NOSAMPLE.  Every source y is 0 and the integer destination x sum to 0, so with the Hartley means exact
    (m1y = 0, m2x = 0) columns 1, 4 and 7 of the normalised system [ux uy u vx vy v x y 1] are exactly zero.  The Jacobi
    sweeps leave zero rows and columns alone, the first zero diagonal (index 1) is the "smallest eigenvalue", F has the one
    entry F[0][1] != 0, F^T F has rank 1 and project_essential refuses it (l2 = 0).  As a fundamental matrix the same F
    scores every row with u != 0 at Sampson error 0.  The sampled modes reject every hypothesis on these columns (a zero
    pivot), so they return nothing before any projection."""
    if model != 4:
        return None
    rng = _rng(model, seed, 19)
    n = 64
    P = np.c_[rng.integers(-20, 21, n), np.zeros(n)].astype(np.float64)
    u = rng.integers(-9, 10, n)
    u[-1] -= u.sum()
    Q = np.c_[u, rng.uniform(-5, 5, n)].astype(np.float64)
    return P, Q, 0.01, ("no_model", "no_model", "projection")


@_register("projection_underflow")
def _projection_underflow(model, seed):
    """Model 4, all three modes: the nominal two-view case times 1e150 (threshold alike).  The Sampson error is scale
    covariant and stays finite (~1e294), so the winner scores its inliers as usual; F = T2^T Fh T1 then has entries of
    1e-300, 1e-150 and 1, its second singular value is far below the 1e-300 floor of project_essential, and the winner is
    refused after it has been scored."""
    if model != 4:
        return None
    P, Q, thr = nominal(4, 300, seed)
    return P * 1e150, Q * 1e150, thr * 1e150, "projection"


# ---------------------------------------------------------------- threshold extremes
def _threshold(thr, expect):
    def build(model, seed):
        P, Q, _ = nominal(model, 300, seed)
        return P, Q, thr, expect
    return build


# 0 and 1e-300 (its square underflows to 0): only exact zeros are inliers.  1e200 (its square overflows) and +inf: every
# defined row is an inlier, so RANSAC's first valid hypothesis already holds the maximum unless it leaves rows undefined.
CLASSES["thr_0"] = _threshold(0.0, ("any", "model", "any"))
CLASSES["thr_1e-300"] = _threshold(1e-300, ("any", "model", "any"))
CLASSES["thr_1e200"] = _threshold(1e200, ("all_inliers", "model", "any"))
CLASSES["thr_inf"] = _threshold(np.inf, ("all_inliers", "model", "any"))


def cases(models=MODELS, seed=0):
    """(class name, model, src, dst, threshold, expect) of every class for every model it applies to."""
    for name, build in CLASSES.items():
        for model in models:
            c = build(model, seed)
            if c is not None:
                yield (name, model) + tuple(c)
