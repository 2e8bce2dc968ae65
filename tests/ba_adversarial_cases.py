"""A census of named bundle-adjustment problems for gh_ba_solve / oracle_ba_solve at the places the friendly graphs of
gslam_amd.ba_synth.make_graph never reach: the chunk and segment boundaries of the kernels (kCamChunk = 1024 observations
of a camera per workgroup, kSchurSeg = 256 pairs of a camera-pair block per wave, 256 points per workgroup, the switch of
the set-up at 20000 observations), degenerate structure (unobserved and single-observation points, cameras without
observations, everything or nothing fixed, one camera, one point, no points, no observations, no iterations, a point
every camera sees, a camera that sees a point twice) and value edges (quaternions that are not unit, dof words with
foreign bits, rank-1 / zero / tiny informations, Huber off / huge / tiny, depths at kMinDepth = 1e-9, observations behind
their cameras, NaN / Inf).

numpy only, inputs only: no expected result comes from this file except YARDSTICK (see there).  CASES maps a name to
{"graph": a dict in the layout of make_graph (+ point_free / obs_info where the case needs them), "huber", "max_iterations"}.
Every solve takes well under a second on either side."""
import numpy as np

from gslam_amd.ba_synth import make_graph

MIN_DEPTH = 1e-9  # kMinDepth of gslam_amd/csrc/ba_obs.h, BA_MIN_DEPTH of oracle/ba_oracle.c
DENSE3 = (255, 256, 257, 1023, 1024, 1025, 2049)
POINT_EDGES = (255, 256, 257)


# ------------------------------------------------------------------------------------------------ float64 restatement
def world_to_cam(pose, X):
    """X_c of the header's contract in plain float64, operation for operation: the quaternion is used as it stands."""
    q = [-float(pose[0]), -float(pose[1]), -float(pose[2]), float(pose[3])]
    p = [float(X[0]) - float(pose[4]), float(X[1]) - float(pose[5]), float(X[2]) - float(pose[6])]
    uvx, uvy, uvz = q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]
    uvx += uvx; uvy += uvy; uvz += uvz
    return np.array([p[0] + q[3] * uvx + (q[1] * uvz - q[2] * uvy), p[1] + q[3] * uvy + (q[2] * uvx - q[0] * uvz),
                     p[2] + q[3] * uvz + (q[0] * uvy - q[1] * uvx)])


def project(pose, X):
    Xc = world_to_cam(pose, X)
    return Xc[:2] / Xc[2]


def depths(g):
    """The camera-frame depth of every observation at the start."""
    return np.array([world_to_cam(g["cam_pose"][c], g["point_xyz"][p])[2] for c, p in zip(g["obs_cam"], g["obs_point"])])


# ------------------------------------------------------------------------------------------------ graph surgery
OBS_KEYS = ("obs_cam", "obs_point", "obs_xy", "obs_info")


def _copy(g):
    return dict((k, np.array(v, copy=True)) for k, v in g.items())


def _keep_obs(g, keep):
    g = _copy(g)
    for k in OBS_KEYS:
        if k in g:
            g[k] = np.ascontiguousarray(g[k][keep])
    return g


def _add_obs(g, cam, point, xy):
    g = _copy(g)
    assert "obs_info" not in g
    g["obs_cam"] = np.concatenate([g["obs_cam"], np.asarray(cam, np.int32)])
    g["obs_point"] = np.concatenate([g["obs_point"], np.asarray(point, np.int32)])
    g["obs_xy"] = np.ascontiguousarray(np.concatenate([g["obs_xy"], np.asarray(xy, np.float64).reshape(-1, 2)]))
    return g


def _add_points(g, xyz):
    g = _copy(g)
    g["point_xyz"] = np.ascontiguousarray(np.concatenate([g["point_xyz"], np.asarray(xyz, np.float64).reshape(-1, 3)]))
    if "point_free" in g:
        g["point_free"] = np.concatenate([g["point_free"], np.ones(len(g["point_xyz"]) - len(g["point_free"]), np.uint8)])
    return g


def _add_cams(g, poses, dof):
    g = _copy(g)
    g["cam_pose"] = np.ascontiguousarray(np.concatenate([g["cam_pose"], np.asarray(poses, np.float64).reshape(-1, 7)]))
    g["cam_dof"] = np.concatenate([g["cam_dof"], np.asarray(dof, np.int32)])
    return g


def _case(g, huber=0.01, max_iterations=12):
    g = dict((k, v) for k, v in g.items() if k in ("cam_pose", "cam_dof", "point_xyz", "point_free", "obs_cam", "obs_point", "obs_xy", "obs_info"))
    return {"graph": g, "huber": huber, "max_iterations": max_iterations}


def base():
    """The good 6-camera graph most cases are cut from: 120 points, four observers each."""
    return make_graph(6, 120, 4, seed=21)


# ------------------------------------------------------------------------------------------------ chunk / segment / switch
def dense3(n):
    return _case(make_graph(3, n, 3, seed=n), max_iterations=12)


def switch(which):
    g = make_graph(4, 5000, 4, seed=3)
    if which == 19999:
        g = _keep_obs(g, np.arange(len(g["obs_cam"])) != 7777)
    elif which == 20001:
        k = 12345
        g = _add_obs(g, [g["obs_cam"][k]], [g["obs_point"][k]], g["obs_xy"][k] + 1e-3)
    return _case(g, max_iterations=10)


def point_edge(n):
    g = make_graph(6, n, 4, seed=100 + n)
    return _case(_keep_obs(g, g["obs_point"] != n - 1))


# ------------------------------------------------------------------------------------------------ structure
def unobserved(fixed):
    rng = np.random.default_rng(31)
    g = base()
    n_points, n_cams = len(g["point_xyz"]), len(g["cam_dof"])
    g["point_free"] = np.ones(n_points, np.uint8)
    g = _add_points(g, rng.uniform(-3, 3, size=(5, 3)))
    extra = g["cam_pose"][2].copy()
    extra[4:] += [0.7, -0.4, 0.3]
    g = _add_cams(g, extra, [0 if fixed else 63])
    if fixed:
        g["point_free"][n_points:] = 0
    assert len(g["cam_dof"]) == n_cams + 1
    return _case(g)


def single_obs_points():
    g = base()
    first = np.ones(len(g["obs_cam"]), bool)
    for p in range(10):
        first[np.flatnonzero(g["obs_point"] == p)[1:]] = False
    return _case(_keep_obs(g, first))


def fixed_variant(cams, points):
    g = base()
    if cams == "fixed":
        g["cam_dof"] = np.zeros(len(g["cam_dof"]), np.int32)
    elif cams == "free":
        g["cam_dof"] = np.full(len(g["cam_dof"]), 63, np.int32)
    if points == "fixed":
        g["point_free"] = np.zeros(len(g["point_xyz"]), np.uint8)
    return _case(g, max_iterations=20 if cams == "free" else 12)


def one_camera(free):
    g = make_graph(1, 40, 3, seed=41)
    if free:
        rng = np.random.default_rng(42)  # make_graph leaves camera 0 at the ground truth: start it off
        g["cam_pose"][0, 4:] += rng.normal(size=3) * 0.05
        g["cam_dof"] = np.array([63], np.int32)
        g["point_free"] = np.zeros(40, np.uint8)
    return _case(g, max_iterations=20)


def two_cams_one_point():
    return _case(make_graph(2, 1, 2, seed=43), max_iterations=20)


def no_points():
    g = make_graph(4, 30, 3, seed=44)
    g = _keep_obs(g, np.zeros(len(g["obs_cam"]), bool))
    g["point_xyz"] = np.zeros((0, 3))
    return _case(g)


def no_obs():
    g = base()
    return _case(_keep_obs(g, np.zeros(len(g["obs_cam"]), bool)))


def hub_point():
    g = make_graph(130, 600, 5, seed=8)
    cams = [c for c in range(130) if world_to_cam(g["cam_pose"][c], g["point_xyz"][0])[2] > 0.5]
    xy = np.array([project(g["cam_pose"][c], g["point_xyz"][0]) for c in cams])
    return _case(_add_obs(g, cams, [0] * len(cams), xy), max_iterations=10)


def same_camera_twice():
    g = make_graph(3, 1100, 3, seed=45)
    ks = np.flatnonzero(g["obs_cam"] == 1)[:30]
    return _case(_add_obs(g, g["obs_cam"][ks], g["obs_point"][ks], g["obs_xy"][ks] + 1e-3))


# ------------------------------------------------------------------------------------------------ values
def nonunit_quat():
    g = base()
    for cam, scale in ((2, 1.3), (3, -1.0), (4, 0.5)):
        g["cam_pose"][cam, :4] *= scale
    return _case(g, max_iterations=20)


EXTRA_DOF = [0, 63 | 64, 127, (1 << 20) | 63, 64, 63]


def extra_dof_bits():
    g = base()
    g["cam_dof"] = np.array(EXTRA_DOF, np.int32)
    return _case(g)


DOF_MASKS = [0, 56, 7, 62, 63, 63]  # camera 1 turns but keeps its translation, camera 2 moves but does not turn


def dof_masks():
    g = base()
    g["cam_dof"] = np.array(DOF_MASKS, np.int32)
    return _case(g)


TINY_INFO_POINTS = 5  # every observation of the points 0 .. 4 carries 1e-8 I: their V diagonal lies under the 1e-6 floor


def rank1_and_zero_info():
    rng = np.random.default_rng(51)
    g = base()
    no = len(g["obs_cam"])
    A = rng.normal(size=(no, 2, 2)) * 0.3 + np.eye(2)
    info = np.einsum("nij,nkj->nik", A, A)           # symmetric positive definite
    v = rng.normal(size=(no, 2))
    rank1 = np.einsum("ni,nj->nij", v, v)
    kind = rng.integers(0, 6, size=no)               # 0: rank 1, 1: zero, else positive definite
    info[kind == 0] = rank1[kind == 0]
    info[kind == 1] = 0.0
    info[g["obs_point"] < TINY_INFO_POINTS] = 1e-8 * np.eye(2)
    g["obs_info"] = np.ascontiguousarray(info.reshape(no, 4))
    return _case(g)


def damping_floor():
    """rank1_and_zero_info stopped after two iterations: the steps of the points 0 .. 4 (V diagonal of 4e-10, a gradient that
    does not vanish) are set by the floor of the damping, clamp(diag, 1e-6, 1e32) / radius, and later iterations, whose
    radius has grown, have not yet taken them to the optimum whatever the floor."""
    case = rank1_and_zero_info()
    case["max_iterations"] = 2
    return case


def zero_info():
    g = base()
    g["obs_info"] = np.zeros((len(g["obs_cam"]), 4))
    return _case(g)


def depth_edge():
    """An extra fixed camera at the origin with the identity rotation, and three extra points in front of it that nothing
    else sees: in that camera's frame X_c = X bit for bit (checked below), so the depths are exactly 0.5e-9, 1e-9 and 2e-9."""
    g = base()
    n_points, n_cams = len(g["point_xyz"]), len(g["cam_dof"])
    cam = np.array([0, 0, 0, 1.0, 0, 0, 0])
    zs = (0.5 * MIN_DEPTH, MIN_DEPTH, 2 * MIN_DEPTH)
    pts = np.array([[0.3 * z, -0.2 * z, z] for z in zs])
    g = _add_cams(g, cam, [0])
    g = _add_points(g, pts)
    xy = pts[:, :2] / pts[:, 2:3] + [[0.002, -0.001]] * 3
    g = _add_obs(g, [n_cams] * 3, [n_points, n_points + 1, n_points + 2], xy)
    for k, z in enumerate(zs):
        assert world_to_cam(cam, pts[k])[2] == z and world_to_cam(cam, pts[k]).tobytes() == pts[k].tobytes()
    return _case(g)


BEHIND = 70


def behind_at_start():
    """70 extra points on the rays through the cameras 1 and 4, beyond them (radius 13 against the cameras' 10): behind
    their own camera by 3, in front of the other three observers by 3.5 and more."""
    rng = np.random.default_rng(61)
    g = base()
    n_points = len(g["point_xyz"])
    cams, pts, xys = [], [], []
    new = np.zeros((BEHIND, 3))
    for i in range(BEHIND):
        own = 1 if i < BEHIND // 2 else 4
        new[i] = 1.3 * g["cam_pose_gt"][own, 4:] + rng.normal(size=3) * 0.3
        for c in (own, (own + 1) % 6, (own + 3) % 6, (own + 5) % 6):
            cams.append(c)
            pts.append(n_points + i)
            xys.append(project(g["cam_pose_gt"][c], new[i]) + rng.normal(size=2) * 0.002 if c != own else np.zeros(2))
    g = _add_points(g, new + rng.normal(size=new.shape) * 0.02)
    return _case(_add_obs(g, cams, pts, np.array(xys)))


# ------------------------------------------------------------------------------------------------ non-finite
def poisoned(what):
    g = base()
    if what == "nan_obs":
        g["obs_xy"][37, 1] = np.nan
    elif what == "inf_obs":
        g["obs_xy"][37, 0] = np.inf
    elif what == "nan_pose":
        g["cam_pose"][3, 5] = np.nan
    elif what == "nan_point":
        g["point_xyz"][11, 0] = np.nan
    return _case(g, max_iterations=30)


NON_FINITE = ("nan_obs", "inf_obs", "nan_pose", "nan_point")


# ------------------------------------------------------------------------------------------------ pose-only LM (gh_ba_pnp)
def pnp_cases():
    """name -> (points n x 3, observations n x 2, start pose, dof) on the 40 points of one_camera_free_points_fixed."""
    g = one_camera(True)["graph"]
    assert np.array_equal(g["obs_point"], np.arange(40))
    X, m, pose = g["point_xyz"], g["obs_xy"], g["cam_pose"][0]
    out = dict(("n%d" % n, (X[:n].copy(), m[:n].copy(), pose, 63)) for n in (0, 1, 2, 3))
    behind = 2 * pose[4:] - X  # mirrored through the camera centre: every depth changes its sign
    assert all(world_to_cam(pose, b)[2] < -1.0 for b in behind)
    out.update({"all_behind": (behind, m, pose, 63), "dof0": (X, m, pose, 0), "dof7": (X, m, pose, 7)})
    return out


PNP_CASES = pnp_cases()
PNP_NOTHING_TO_DO = ("n0", "all_behind", "dof0")  # 0 iterations, termination 2, the pose bit for bit


def build():
    cases = {}
    for n in DENSE3:
        cases["dense3_%d" % n] = dense3(n)
    for n in (19999, 20000, 20001):
        cases["switch_%d" % n] = switch(n)
    for n in POINT_EDGES:
        cases["points_%d" % n] = point_edge(n)
    cases.update({
        "unobserved": unobserved(False), "unobserved_fixed": unobserved(True), "single_obs_points": single_obs_points(),
        "all_cams_fixed": fixed_variant("fixed", "free"), "all_points_fixed": fixed_variant("as_is", "fixed"),
        "everything_fixed": fixed_variant("fixed", "fixed"), "gauge_free": fixed_variant("free", "free"),
        "one_camera_fixed": one_camera(False), "one_camera_free_points_fixed": one_camera(True),
        "two_cams_one_point": two_cams_one_point(), "no_points": no_points(), "no_obs": no_obs(),
        "zero_iterations": _case(base(), max_iterations=0), "hub_point": hub_point(), "same_camera_twice": same_camera_twice(),
        "nonunit_quat": nonunit_quat(), "extra_dof_bits": extra_dof_bits(), "dof_masks": dof_masks(), "rank1_and_zero_info": rank1_and_zero_info(),
        "damping_floor": damping_floor(), "zero_info": zero_info(), "huber_off": _case(base(), huber=0.0), "huber_negative": _case(base(), huber=-1.0),
        "huber_1e300": _case(base(), huber=1e300), "huber_1e-300": _case(base(), huber=1e-300),
        "depth_edge": depth_edge(), "behind_at_start": behind_at_start()})
    for what in NON_FINITE:
        cases[what] = poisoned(what)
    return cases


CASES = build()
NAMES = list(CASES)
FINITE = [n for n in NAMES if n not in NON_FINITE]
# gate-only classes: the solve stops before a step is taken and the state comes back bit for bit
NOTHING_TO_DO = ("everything_fixed", "no_points", "no_obs", "zero_info", "huber_1e-300")   # 0 iterations, termination 2
BOTH_MODES = ["dense3_%d" % n for n in DENSE3] + ["switch_%d" % n for n in (19999, 20000, 20001)] + ["hub_point"]


def fixed_cams(g):
    return [int(c) for c in np.flatnonzero((np.asarray(g["cam_dof"]) & 63) == 0)]


def fixed_points(g):
    return [] if g.get("point_free") is None else [int(p) for p in np.flatnonzero(np.asarray(g["point_free"]) == 0)]


def unobserved_points(g):
    return [int(p) for p in np.flatnonzero(np.bincount(g["obs_point"], minlength=len(g["point_xyz"])) == 0)]


def unobserved_cams(g):
    return [int(c) for c in np.flatnonzero(np.bincount(g["obs_cam"], minlength=len(g["cam_dof"])) == 0)]


# The largest difference of the final state (poses and points) between the oracle and the oracle compiled with FMA contraction
# (oracle/liboracle_fma.so: the same source, other roundings), per finite case: how far rounding alone moves each solution.
# tests/test_ba_adversarial_oracle.py::test_yardstick re-measures every figure and holds it within 2 x of this table;
# tests/test_ba_adversarial_gpu.py takes its state bar from it: max(1e-8, 8 x the case's figure).
YARDSTICK = {
    "dense3_255": 1.11e-14,
    "dense3_256": 1.15e-14,
    "dense3_257": 5.33e-15,
    "dense3_1023": 7.99e-15,
    "dense3_1024": 1.07e-14,
    "dense3_1025": 5.33e-15,
    "dense3_2049": 1.42e-14,
    "switch_19999": 4.44e-15,
    "switch_20000": 3.55e-15,
    "switch_20001": 3.94e-15,
    "points_255": 3.55e-15,
    "points_256": 9.55e-15,
    "points_257": 5.33e-15,
    "unobserved": 3.77e-15,
    "unobserved_fixed": 3.77e-15,
    "single_obs_points": 5.26e-11,
    "all_cams_fixed": 2.78e-15,
    "all_points_fixed": 1.78e-15,
    "everything_fixed": 0.0,
    "gauge_free": 3.63e-06,
    "one_camera_fixed": 1.48e-11,
    "one_camera_free_points_fixed": 8.88e-16,
    "two_cams_one_point": 1.28e-13,
    "no_points": 0.0,
    "no_obs": 0.0,
    "zero_iterations": 0.0,
    "hub_point": 7.69e-10,
    "same_camera_twice": 5.88e-15,
    "nonunit_quat": 5.51e-14,
    "extra_dof_bits": 2.66e-15,
    "dof_masks": 3.58e-15,
    "rank1_and_zero_info": 7.15e-10,
    "damping_floor": 8.97e-13,
    "zero_info": 0.0,
    "huber_off": 1.42e-14,
    "huber_negative": 1.42e-14,
    "huber_1e300": 1.42e-14,
    "huber_1e-300": 0.0,
    "depth_edge": 3.77e-15,
    "behind_at_start": 1.62e-14,
}
