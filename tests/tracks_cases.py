"""Census inputs of gh_triangulate_tracks_dev: 33 small named points, each built to reach one thing in the contract
(tests/test_tracks_cpu.py shows with the restatement that each does), in one call.  33 points fill neither the second wave
nor the second workgroup of the launch.  The observation arrays interleave the tracks, in descending point order; the call has
to build the index itself."""
import functools

import numpy as np

import tracks_restate as tr

FILL_XYZ = 7.0     # what the output buffers hold on entry
FILL_BYTE = 0xAB
FILL_INT = -5
PARAMS = dict(tr.DEFAULTS)  # min_parallax_cos 0.9998, max_reproj 0.004, min_views 2, max_drops 2
OUTLIER = (0.3, -0.2)       # added to an exact projection: 90 times the reprojection bound
LONG = 600                  # 75 trips of a group of 8 lanes
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _quat(axis, angle):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    return np.r_[a * np.sin(angle / 2), np.cos(angle / 2)]


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _project(pose, X):
    """Through the pinhole whatever the sign of the depth: the LINE of the observation passes through X."""
    Xc = _rot(pose[:4]).T @ (np.asarray(X, float) - pose[4:7])
    return Xc[:2] / Xc[2]


def cameras():
    """0 .. 23 a row of cameras 0.5 apart, each turned a little; 24 .. 26 three cameras with one pose; 27 a NaN in the
    quaternion; 28 .. 30 a row 0.01 apart (below the parallax bound at depth 6); 31 at the origin with -0.0 in its translation;
    32, 33 look AWAY from the scene (what they observe lies behind them); 34 a NaN in the translation."""
    cams = []
    for c in range(24):
        q = _quat([0.2, 1.0, 0.1 * (c % 3)], -0.03 * (c - 12) + 0.01)
        cams.append(np.r_[q, 0.5 * c - 6.0 + 0.03 * (c % 5), 0.1 * np.sin(c), 0.05 * (c % 4)])
    same = np.r_[_quat([0, 1, 0], 0.05), 1.0, 0.5, -0.25]
    cams += [same.copy(), same.copy(), same.copy()]
    cams.append(np.r_[0.0, NAN_, 0.0, 1.0, 0.0, 0.0, 0.0])
    for k in range(3):
        cams.append(np.r_[_quat([0, 0, 1], 0.02 * k), 0.01 * k, 0.0, 0.0])
    cams.append(np.array([0.0, 0.0, 0.0, 1.0, -0.0, -0.0, 0.0]))
    cams.append(np.r_[_quat([0, 1, 0], np.pi - 0.1), -2.0, 0.3, 0.0])
    cams.append(np.r_[_quat([0, 1, 0], np.pi + 0.15), 2.5, -0.2, 0.1])
    cams.append(np.r_[_quat([0, 1, 0], 0.02), 1.0, NAN_, 0.0])
    return np.array(cams)


NAN_ = float("nan")
N_CAMS = 35


@functools.lru_cache(maxsize=None)
def _build():
    rng = np.random.default_rng(20)
    cam = cameras()
    assert len(cam) == N_CAMS
    names, tracks, select = [], [], []   # tracks[p]: list of [cam, x, y, use, point index to store]

    def X_of(p):
        return np.array([0.7 * np.sin(1.3 * p), 0.5 * np.cos(0.7 * p), 6.0 + 0.25 * (p % 7)])

    def add(name, cams, outliers=(), noise=2e-4, X=None, sel=1):
        p = len(names)
        X = X_of(p) if X is None else np.asarray(X, float)
        obs = []
        for r, c in enumerate(cams):
            xy = _project(cam[c], X) + rng.standard_normal(2) * noise
            if r in outliers:
                xy = xy + np.array(OUTLIER)
            obs.append([int(c), float(xy[0]), float(xy[1]), 1, p])
        names.append(name)
        tracks.append(obs)
        select.append(sel)
        return obs

    row = lambda n, first=0, step=1: [(first + step * k) % 24 for k in range(n)]
    add("len0", [])
    add("len1", [3])
    add("len2", [2, 9])
    add("len7", row(7, 1, 3))
    add("len8", row(8, 0, 3))
    add("len9", row(9, 2, 2))
    add("len16", row(16, 0, 1))
    add("len17", row(17, 5, 1))
    add("len600_drop1", row(LONG, 0, 5), outliers=(300,))
    add("drop1", row(6, 4, 3), outliers=(2,))
    add("drop2", row(7, 0, 3), outliers=(1, 5))
    add("three_outliers", row(9, 1, 2), outliers=(0, 4, 7))
    add("two_skew_rays", [5, 14], outliers=(1,))           # bad with min_views members: INCONSISTENT without a drop
    add("stop_at_min_views", [3, 11, 19], outliers=(0, 2))  # one drop, then the live set has min_views members
    add("tie_behind", [32, 4, 33, 12, 20], noise=0.0)       # ranks 0 and 2 behind their cameras: two +inf keys
    o = add("nan_xy", row(4, 6, 4))
    o[2][1] = NAN_
    o = add("nan_pose", [8, 27, 15])
    o[1][1], o[1][2] = 0.1, -0.05   # (the NaN is in the pose alone)
    add("same_centre", [24, 25, 26], noise=0.0)
    add("low_parallax", [28, 29, 30], X=[0.2, -0.1, 6.0], noise=1e-6)
    add("anchor_dropped_low", [2, 28, 29, 30], outliers=(0,), X=[0.2, -0.1, 6.0], noise=1e-6)
    add("anchor_dropped_ok", row(5, 7, 3), outliers=(0,))
    o = add("duplicate", row(3, 3, 6))
    o.append(list(o[1]))
    o = add("neg_zero", [31, 10, 17], X=[-0.0, -0.0, 6.0], noise=0.0)
    o[0][1] = o[0][2] = -0.0
    o = add("masked_outliers", row(5, 2, 4), outliers=(1, 3))
    o[1][3] = o[3][3] = 0
    o = add("masked_too_few", [6, 13])
    o[0][3] = 0
    add("skipped", row(4, 0, 5), sel=0)
    add("skipped_empty", [], sel=0)
    o = add("bad_cam_index", row(7, 1, 3))
    for r, c in ((0, -1), (2, N_CAMS), (4, INT_MAX), (6, INT_MIN)):
        o[r][0] = c
    o = add("bad_point_index", row(6, 3, 3))
    for r, q in ((1, -1), (3, 33), (4, INT_MAX), (5, INT_MIN)):  # four observations that belong to no point: two are left
        o[r][4] = q
    # a NaN in a translation leaves the pivots regular: X is NaN, nobody is good, every key is +inf, the lowest rank goes
    o = add("nan_translation", [8, 34, 15, 20, 2])
    o[1][1], o[1][2] = -0.02, 0.03
    add("outlier_rank7", row(8, 3, 2), outliers=(7,))
    add("outlier_rank8", row(9, 5, 2), outliers=(8,))
    add("two_in_one_lane", row(17, 0, 1), outliers=(8, 16))
    assert len(names) == 33
    # the call's arrays: rank by rank, the points in descending order
    rows = []
    for r in range(max(len(t) for t in tracks)):
        for p in reversed(range(len(tracks))):
            if r < len(tracks[p]):
                rows.append(tracks[p][r])
    return dict(names=names, n_points=len(names), cam_pose=np.ascontiguousarray(cam),
                obs_cam=np.array([o[0] for o in rows], np.int32), obs_point=np.array([o[4] for o in rows], np.int32),
                obs_xy=np.array([[o[1], o[2]] for o in rows], np.float64), obs_use=np.array([o[3] for o in rows], np.uint8),
                point_select=np.array(select, np.uint8))


def arrays():
    """-> dict: names, n_points, cam_pose, obs_cam, obs_point, obs_xy, obs_use, point_select (host arrays; do not modify)."""
    return _build()


def index(name):
    return _build()["names"].index(name)


@functools.lru_cache(maxsize=None)
def expected():
    """The restatement on the census, output buffers filled as the GPU test fills them.  Computed once; do not modify."""
    a = _build()
    return tr.tracks(a["cam_pose"].tolist(), a["obs_cam"].tolist(), a["obs_point"].tolist(), a["obs_xy"].tolist(), a["n_points"],
                     a["obs_use"].tolist(), a["point_select"].tolist(), [[FILL_XYZ] * 3] * a["n_points"], **PARAMS)


GRAPH_PARAMS = {False: dict(PARAMS, max_reproj=1e-9), True: dict(PARAMS, max_reproj=0.01, max_drops=2)}


@functools.lru_cache(maxsize=None)
def graph(noisy):
    """40 cameras, 2000 points, 6 observations each, the cameras at ground truth.  noisy False: exact observations; True: pixel
    noise 0.002 and the generator's 5 % outliers.  -> the dict of ba_synth.make_graph (do not modify)."""
    from gslam_amd.ba_synth import make_graph
    if noisy:
        return make_graph(40, 2000, 6, seed=3, noise=0.002, perturb=False)
    return make_graph(40, 2000, 6, seed=3, noise=0, outlier_frac=0, perturb=False)


@functools.lru_cache(maxsize=None)
def graph_expected(noisy):
    """The restatement on graph(noisy) under GRAPH_PARAMS[noisy].  Computed once; do not modify."""
    g = graph(noisy)
    return tr.tracks(g["cam_pose"].tolist(), g["obs_cam"].tolist(), g["obs_point"].tolist(), g["obs_xy"].tolist(),
                     len(g["point_xyz"]), **GRAPH_PARAMS[noisy])


def permuted(a, seed):
    """The same tracks in another interleaving: a random merge that keeps the order inside every track.  -> (arrays, perm)
    with new[i] = old[perm[i]]."""
    rng = np.random.default_rng(seed)
    n = len(a["obs_cam"])
    # (an observation with a bad point index belongs to no track: it may go anywhere)
    key = np.where((a["obs_point"] >= 0) & (a["obs_point"] < a["n_points"]), a["obs_point"], -1).astype(np.int64)
    slots = rng.permutation(n)
    perm = np.empty(n, np.int64)
    for k in np.unique(key):
        members = np.flatnonzero(key == k)          # ascending: the track order
        where = np.sort(slots[members])             # the slots this track gets, ascending
        perm[where] = members
    b = dict(a)
    for k in ("obs_cam", "obs_point", "obs_xy", "obs_use"):
        b[k] = np.ascontiguousarray(a[k][perm])
    return b, perm
