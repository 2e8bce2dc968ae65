"""Inputs for gh_ba_window_dev: a hand-built census (8 cameras, 12 points, 34 named observations), a random soup at the block
boundaries of every launch (n_obs 512 / 513, n_cams 256 / 257, n_points 512 / 513), a hub (one point seen from 257 cameras, one
camera with 3001 observations) and a 60-camera trajectory whose last two frames are new.  tests/test_ba_window_cpu.py shows
what they reach; tests/test_ba_window_gpu.py holds the device to tests/ba_window_restate.py on them, byte for byte."""
import functools

import numpy as np

import ba_window_restate as rs

INT32_MAX = 2**31 - 1
OUTPUTS = ("cam_class", "cam_shared", "cam_slot", "point_slot", "win_cam", "win_cam_dof", "win_cam_pose", "win_point", "win_point_xyz",
           "win_obs_cam", "win_obs_point", "win_obs_src", "win_obs_xy", "totals")
DTYPE = dict(cam_class=np.uint8, cam_shared=np.int32, cam_slot=np.int32, point_slot=np.int32, win_cam=np.int32, win_cam_dof=np.int32,
             win_cam_pose=np.float64, win_point=np.int32, win_point_xyz=np.float64, win_obs_cam=np.int32, win_obs_point=np.int32,
             win_obs_src=np.int32, win_obs_xy=np.float64, totals=np.int32)
OBS_OUTPUTS = ("win_obs_cam", "win_obs_point", "win_obs_src", "win_obs_xy")


def sizes(n_cams, n_points, n_obs):
    """Bytes of every output at its capacity."""
    return dict(cam_class=n_cams, cam_shared=4 * n_cams, cam_slot=4 * n_cams, point_slot=4 * n_points, win_cam=4 * n_cams,
                win_cam_dof=4 * n_cams, win_cam_pose=56 * n_cams, win_point=4 * n_points, win_point_xyz=24 * n_points,
                win_obs_cam=4 * n_obs, win_obs_point=4 * n_obs, win_obs_src=4 * n_obs, win_obs_xy=16 * n_obs, totals=32)


def _values(n_cams, n_points, n_obs, seed):
    """Poses, points and measurements whose bits tell the rows apart (no geometry: the window copies bits)."""
    rng = np.random.default_rng(seed)
    return dict(cam_pose=rng.standard_normal((n_cams, 7)), point_xyz=rng.standard_normal((n_points, 3)),
                obs_xy=rng.standard_normal((n_obs, 2)))


# name, camera, point, obs_use -- min_shared = 3, min_point_obs = 2.  What every row is for:
#   cameras  7 seed, LOCAL.  6 seed and held, LOCAL (shared 2 < min_shared: a seed needs one).  5 seed WITHOUT a live observation: NONE
#            (its observation of point 0 has obs_use 0, its other one is of a point that is not live).  4 shared == min_shared
#            exactly, and only because the pair (4, 1) is given twice: LOCAL.  3 held, shared 3: LOCAL with dof 0.  2 shared ==
#            min_shared - 1 and sees window points: FIXED.  1 sees only points outside the window: NONE.  0 held, sees the window
#            point 4: FIXED (held changes nothing there).
#   points   0 .. 3 SEEN (camera 7).  4 exactly min_point_obs observations, in the window through LOCAL camera 4, not SEEN.  5 live,
#            cameras 1 and 0: no LOCAL camera, outside.  6 live only because (1, 6) is given twice; seen only by NONE cameras.
#            7 exactly min_point_obs - 1 usable observations (its second has obs_use 0): not live.  8 point_use 0, though two seeds
#            see it.  9 one observation, in a seed.  10 live, cameras 3 and 2, in the window, not SEEN.  11 nowhere.
CENSUS_ROWS = [
    ("seed7_p0", 7, 0, 1), ("seed7_p1", 7, 1, 1), ("cam4_p0", 4, 0, 1), ("bad_cam_minus1", -1, 0, 1), ("seed6_p0", 6, 0, 1),
    ("cam4_p1_first", 4, 1, 1), ("cam1_p6_first", 1, 6, 1), ("seed7_p2", 7, 2, 1), ("bad_cam_n", 8, 1, 1), ("cam3_p1", 3, 1, 1),
    ("seed5_p0_unused", 5, 0, 0), ("seed7_p3", 7, 3, 1), ("cam2_p2", 2, 2, 1), ("bad_point_minus1", 7, -1, 1), ("cam4_p1_again", 4, 1, 1),
    ("seed6_p1", 6, 1, 1), ("cam3_p2", 3, 2, 1), ("seed7_p8_point_unused", 7, 8, 1), ("cam0_p4", 0, 4, 1), ("bad_point_n", 7, 12, 1),
    ("cam2_p3", 2, 3, 1), ("seed5_p7_short", 5, 7, 1), ("cam3_p3", 3, 3, 1), ("seed7_p7_unused", 7, 7, 0), ("cam4_p4", 4, 4, 1),
    ("cam1_p5", 1, 5, 1), ("seed6_p8_point_unused", 6, 8, 1), ("cam0_p5", 0, 5, 1), ("bad_cam_int_max", INT32_MAX, 2, 1),
    ("seed7_p9_single", 7, 9, 1), ("cam3_p10", 3, 10, 1), ("bad_point_int_min", 6, -INT32_MAX - 1, 1), ("cam1_p6_again", 1, 6, 1),
    ("cam2_p10", 2, 10, 1),
]


def census():
    n_cams, n_points, n_obs = 8, 12, len(CENSUS_ROWS)
    point_use = np.ones(n_points, np.uint8)
    point_use[8] = 0
    cam_seed = np.array([0, 0, 0, 0, 0, 9, 1, 255], np.uint8)
    cam_hold = np.array([1, 0, 0, 7, 0, 0, 1, 0], np.uint8)
    return dict(name="census", n_cams=n_cams, n_points=n_points, obs_cam=np.array([r[1] for r in CENSUS_ROWS], np.int32),
                obs_point=np.array([r[2] for r in CENSUS_ROWS], np.int32), obs_use=np.array([r[3] * 3 for r in CENSUS_ROWS], np.uint8),
                point_use=point_use, cam_seed=cam_seed, cam_hold=cam_hold, min_shared=3, min_point_obs=2, rows=[r[0] for r in CENSUS_ROWS],
                **_values(n_cams, n_points, n_obs, 41))


def soup(n_cams, n_points, n_obs, seed=11, min_shared=3):
    """Random everything, valid or not.  Seven tenths of the observations fall on six points near their camera, so that
    neighbouring cameras share points; four seeds, a few held cameras; camera and point indices also from the values the
    contract must turn down.  The first and the last observation are live observations of seed cameras: the first and the last
    lane of the range both emit."""
    rng = np.random.default_rng(seed)
    bad = np.array([-1, -2, n_cams, n_cams + 1, INT32_MAX, -INT32_MAX - 1], np.int64)
    obs_cam = np.where(rng.random(n_obs) < 0.04, bad[rng.integers(0, len(bad), n_obs)], rng.integers(0, n_cams, n_obs))
    badp = np.array([-1, -3, n_points, n_points + 7, INT32_MAX, -INT32_MAX - 1], np.int64)
    near = (np.clip(obs_cam, 0, n_cams - 1) * n_points // n_cams + rng.integers(0, 6, n_obs)) % n_points
    obs_point = np.where(rng.random(n_obs) < 0.7, near, rng.integers(0, n_points, n_obs))
    obs_point = np.where(rng.random(n_obs) < 0.04, badp[rng.integers(0, len(badp), n_obs)], obs_point)
    obs_use = (rng.random(n_obs) < 0.85).astype(np.uint8) * rng.integers(1, 256, n_obs).astype(np.uint8)
    point_use = (rng.random(n_points) < 0.9).astype(np.uint8) * rng.integers(1, 256, n_points).astype(np.uint8)
    cam_seed = np.zeros(n_cams, np.uint8)
    cam_seed[[0, n_cams // 3, n_cams - 2, n_cams - 1]] = [1, 2, 128, 255]
    cam_hold = (rng.random(n_cams) < 0.2).astype(np.uint8)
    cam_hold[n_cams - 1] = 1
    point_use[[0, n_points - 1]] = 1
    for k, c, p in ((0, 0, n_points - 1), (1, n_cams - 1, n_points - 1), (n_obs - 2, 0, 0), (n_obs - 1, n_cams - 1, 0)):
        obs_cam[k], obs_point[k], obs_use[k] = c, p, 1
    return dict(name="soup_%dx%dx%d" % (n_cams, n_points, n_obs), n_cams=n_cams, n_points=n_points, obs_cam=obs_cam.astype(np.int32),
                obs_point=obs_point.astype(np.int32), obs_use=obs_use, point_use=point_use, cam_seed=cam_seed, cam_hold=cam_hold,
                min_shared=min_shared, min_point_obs=2, **_values(n_cams, n_points, n_obs, seed + 1))


def boundaries():
    """One workgroup (or two) exactly and one entry more, for every count a launch is sized by; the scan covers
    max(n_obs, n_cams + n_points) + 1 entries: 513 / 514 in the first pair."""
    return [soup(40, 100, 512), soup(40, 100, 513), soup(256, 90, 1500, min_shared=2), soup(257, 90, 1500, min_shared=2),
            soup(40, 512, 1500), soup(40, 513, 1500)]


def hub(order="frame_major"):
    """257 cameras, 3001 points, 6257 observations, min_shared = 13.  Point 0 has one observation in each of the 257 cameras; the
    seed camera 256 sees every point: 3001 observations, more than a workgroup's lanes; point p >= 1 is also seen by camera
    p % 256.  So n_use[0] = 257, shared[256] = 3001, and camera c < 256 shares 1 + (12 if 1 <= c <= 184 else 11) points with the seed:
    cameras 1 .. 184 are LOCAL with shared == min_shared exactly, the other 71 are FIXED with min_shared - 1.  frame_major:
    sorted by camera (runs of one camera); track_major: sorted by point (the hub's 257 observations are one run)."""
    n_cams, n_points = 257, 3001
    cam = list(range(256)) + [256] * 3001
    pt = [0] * 256 + list(range(3001))
    for p in range(1, 3001):
        cam.append(p % 256)
        pt.append(p)
    cam, pt = np.array(cam, np.int64), np.array(pt, np.int64)
    idx = np.lexsort((pt, cam)) if order == "frame_major" else np.lexsort((cam, pt))
    cam_seed = np.zeros(n_cams, np.uint8)
    cam_seed[256] = 1
    cam_hold = np.zeros(n_cams, np.uint8)
    cam_hold[[0, 1, 256]] = 1
    n_obs = len(cam)
    return dict(name="hub_" + order, n_cams=n_cams, n_points=n_points, obs_cam=cam[idx].astype(np.int32), obs_point=pt[idx].astype(np.int32),
                obs_use=np.ones(n_obs, np.uint8), point_use=np.ones(n_points, np.uint8), cam_seed=cam_seed, cam_hold=cam_hold, min_shared=13,
                min_point_obs=2, **_values(n_cams, n_points, n_obs, 51))


TRAJECTORY_SEEDS = (58, 59)
# min_shared -> LOCAL, FIXED, window points, window observations (of 6000): from a numpy restatement of the rule
TRAJECTORY_FIGURES = {15: (9, 8, 305, 1220), 1: (10, 8, 331, 1324)}


@functools.lru_cache(maxsize=None)
def _trajectory_graph(perturb):
    from gslam_amd import ba_synth
    return ba_synth.make_graph(60, 1500, 4, seed=3, noise=0.002, perturb=perturb, covis_window=9)


def trajectory(min_shared=15, perturb=False):
    """60 cameras on a trajectory, 1500 points of 4 observations in windows of 9 cameras; the last two frames are new; frame 0
    would be held, far outside the window.  Every observation is usable."""
    g = _trajectory_graph(perturb)
    n_cams, n_points, n_obs = 60, 1500, len(g["obs_cam"])
    cam_seed = np.zeros(n_cams, np.uint8)
    cam_seed[list(TRAJECTORY_SEEDS)] = 1
    cam_hold = np.zeros(n_cams, np.uint8)
    cam_hold[0] = 1
    return dict(name="trajectory_%d%s" % (min_shared, "_perturbed" if perturb else ""), n_cams=n_cams, n_points=n_points,
                obs_cam=g["obs_cam"].astype(np.int32), obs_point=g["obs_point"].astype(np.int32), obs_use=np.ones(n_obs, np.uint8),
                point_use=np.ones(n_points, np.uint8), cam_seed=cam_seed, cam_hold=cam_hold, min_shared=min_shared, min_point_obs=2,
                cam_pose=np.ascontiguousarray(g["cam_pose"]), point_xyz=np.ascontiguousarray(g["point_xyz"]),
                obs_xy=np.ascontiguousarray(g["obs_xy"]))


def reorder(c, order, seed=0):
    """The same case with its observations in another order (forward, reversed, shuffled) -> (case, perm) with
    new[i] = old[perm[i]].  Unlike tracks_cases.permuted, nothing is kept in place: the window depends on no order at all."""
    n = len(c["obs_cam"])
    perm = {"forward": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "shuffled": np.random.default_rng(seed).permutation(n)}[order]
    d = dict(c, name=c["name"] + "_" + order)
    for k in ("obs_cam", "obs_point", "obs_xy", "obs_use"):
        d[k] = np.ascontiguousarray(c[k][perm])
    return d, perm


def in_source_order(a, perm):
    """The observation outputs of a reordered case (arrays at capacity) as rows sorted by the ORIGINAL observation index:
    (original index, compact camera, compact point, xy bits)."""
    n = int(a["totals"][5])
    src = perm[a["win_obs_src"][:n]]
    order = np.argsort(src, kind="stable")
    return (src[order].tolist(), a["win_obs_cam"][:n][order].tolist(), a["win_obs_point"][:n][order].tolist(),
            np.ascontiguousarray(a["win_obs_xy"].reshape(-1, 2)[:n][order]).tobytes())


def restate(c, use_obs_use=True, use_point_use=True, use_hold=True, min_shared=None, min_point_obs=None):
    """tests/ba_window_restate.py on a case -> its dict of lists and sets."""
    return rs.window(c["n_cams"], c["n_points"], c["cam_pose"].tolist(), c["point_xyz"].tolist(), c["obs_cam"].tolist(),
                     c["obs_point"].tolist(), c["obs_xy"].tolist(), c["cam_seed"].tolist(),
                     c["obs_use"].tolist() if use_obs_use else None, c["point_use"].tolist() if use_point_use else None,
                     c["cam_hold"].tolist() if use_hold else None, c["min_shared"] if min_shared is None else min_shared,
                     c["min_point_obs"] if min_point_obs is None else min_point_obs)


def as_arrays(e):
    """The restatement's lists as the arrays the device writes (flat, at capacity)."""
    return {k: np.array(e[k], DTYPE[k]).reshape(-1) for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def restated(which):
    """Restatements that several tests share, computed once per session and left unchanged."""
    c = {"hub": hub, "trajectory_15": lambda: trajectory(15), "trajectory_1": lambda: trajectory(1)}[which]()
    return c, as_arrays(restate(c))
