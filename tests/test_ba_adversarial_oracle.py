"""The bundle-adjustment oracle (oracle/ba_oracle.c) on the census of tests/ba_adversarial_cases.py, against references
that are independent of it.  The kernels are held to the oracle in tests/test_ba_adversarial_gpu.py; where the two share
a formula only this file can find it wrong.

Census.  From the inputs alone (numpy): observations per camera and chunks of 1024, pairs and segments of 256 per lower
block of the reduced camera system (block (ci >= cj) holds sum_p n_p(ci) n_p(cj) pairs, n_p(c) = observations of point p
in camera c: the definition of the pair list in gslam_amd/csrc/ba.hip), observers per point, n_obs -- and every case is
shown to reach what it is named for (STRUCTURE below; a case without an entry fails the test).

Oracle runs.  Every case returns status 0 and lowers the cost, except the gate-only classes, of which only the gate is
asserted: everything_fixed / no_points / no_obs / zero_info / huber_1e-300 take 0 iterations with termination 2;
zero_iterations ends with termination 0; nan_obs / inf_obs fail (status 1, termination 3) after 15 rejected iterations
whose candidate cost is inf, from an initial cost of NaN -- and all of these return the state bit for bit.  nan_pose /
nan_point return status 0, the NaN stays in its pose / point and nowhere else.  Fixed cameras, fixed points and
unobserved blocks come back bit for bit everywhere.

Linearisation.  oracle_ba_obs_linearize against a 50-digit mpmath evaluation: X_c = M(q)^T (X - t) with
M(q) = I + 2 w [v]x + 2 [v]x^2 (the quaternion as it stands: for a unit q this is the rotation), the Jacobians as central
differences (h = 1e-20) of pi(exp(xi)^-1 (X_c + M^T dX)) with mpmath's own matrix exponential, the Huber weight from its
definition.  For a quaternion that is not unit this is what the header's "used as it stands" means: the camera-frame
perturbation, no normalisation.  Error = max |oracle - mpmath| / max(1, max |mpmath|) per quantity (r, Jc, Jp, w).
Measured worst per class (test_linearisation_against_mpmath prints them); the bar of a class is 8 x its measured
worst, and no bar exceeds 1e-9:
    base (60 observations of the good graph)                  1.5e-14   bar 1.2e-13
    depth_edge (depth 2e-9: Jacobians of 5e8)                 2.2e-16   bar 1.8e-15   <- one ulp: nothing measurable
    nonunit_quat (q x 1.3, x -1, x 0.5)                       1.4e-14   bar 1.1e-13
    rank1_info (rank-1 and zero informations, Huber on)       4.0e-15   bar 3.2e-14
    huber_edge (s at delta^2 and one ulp either side)         2.2e-16   bar 1.8e-15   <- one ulp: nothing measurable
A figure is never recorded below 2^-52 (one ulp of a number of size 1): a float64 result cannot be told apart more finely.
Four of the nonunit_quat observations (camera 4, q x 0.5) lie behind their camera under M(q) on both sides.

First LM step.  The full Jacobian from oracle_ba_obs_linearize in numpy longdouble, the documented damping
clamp(diag, 1e-6, 1e32) / radius, dof masks as removed columns, a dense elimination of the damped normal equations (no
Schur complement), the oracle's exported retraction: the candidate's cost against trace_cost[0].  Measured relative
difference (test_first_lm_step_without_schur prints it); bar = 8 x measured, at most 1e-9:
    unobserved            7.1e-16   bar 5.7e-15
    single_obs_points     8.2e-16   bar 6.6e-15
    all_cams_fixed        2.2e-16   bar 1.8e-15   <- one ulp: the two costs are the same float64
    rank1_and_zero_info   5.6e-15   bar 4.5e-14

Yardstick.  Every finite case through oracle/liboracle.so and oracle/liboracle_fma.so (the same source with FMA contraction):
identical accept / reject sequences, and the largest state difference per case within 2 x of ba_adversarial_cases.YARDSTICK,
which the GPU file takes its state bars from (max(1e-8, 8 x the figure)).  Measured (test_yardstick prints every case):
    dense3_*, switch_*, points_*, same_camera_twice            3.6e-15 .. 1.4e-14
    the structural and value cases on the 6-camera graph       8.9e-16 .. 5.5e-14   (0 where no step is taken)
    damping_floor 9.0e-13   two_cams_one_point 1.3e-13   one_camera_fixed 1.5e-11   single_obs_points 5.3e-11
    rank1_and_zero_info 7.2e-10 (the points that carry 1e-8 of information)   hub_point 7.7e-10
    gauge_free 3.6e-6 (the null space of the free gauge carries the rounding)

The census also holds dof_masks (translation-only and rotation-only cameras: a masked translation
comes back bit for bit), zero_info (every information matrix zero: nothing to do) and damping_floor (rank1_and_zero_info
stopped after two iterations, where the 1e-6 floor of the damping still shows in the state)."""
import ctypes as C
import os

import numpy as np
import pytest

import ba_adversarial_cases as bc
import oracle_lib

LIN_BAR = {"base": 8 * 1.5e-14, "depth_edge": 8 * 2.0 ** -52, "nonunit_quat": 8 * 1.4e-14, "rank1_info": 8 * 4.0e-15,
           "huber_edge": 8 * 2.0 ** -52}
STEP_BAR = {"unobserved": 8 * 7.1e-16, "single_obs_points": 8 * 8.2e-16, "all_cams_fixed": 8 * 2.0 ** -52,
            "rank1_and_zero_info": 8 * 5.6e-15}
ULP = 2.0 ** -52  # the resolution of every measured figure: the relative difference of two float64 numbers
assert max(LIN_BAR.values()) <= 1e-9 and max(STEP_BAR.values()) <= 1e-9


def _opts(case, max_iterations=None):
    return oracle_lib.ba_options(huber=case["huber"], max_iterations=case["max_iterations"] if max_iterations is None else max_iterations)


# ------------------------------------------------------------------------------------------------ census
def census(g):
    nc, npnt = len(g["cam_dof"]), len(g["point_xyz"])
    per_cam = np.bincount(g["obs_cam"], minlength=nc)
    per_point = np.bincount(g["obs_point"], minlength=npnt)
    M = np.zeros((npnt, nc), np.int64)
    np.add.at(M, (g["obs_point"], g["obs_cam"]), 1)
    pairs = np.tril(M.T @ M)
    blocks = pairs[pairs > 0]
    return {"n_cams": nc, "n_points": npnt, "n_obs": len(g["obs_cam"]), "per_cam": per_cam, "chunks": -(-per_cam // 1024),
            "per_point": per_point, "pairs": pairs, "blocks": blocks, "segs": -(-blocks // 256), "span": _span(g, M)}


def _span(g, M):
    seen = [np.flatnonzero(row) for row in M]
    return max([int(s[-1] - s[0]) for s in seen if len(s)] or [0])


def _dense3(n):
    def check(c, g):
        return (list(c["per_cam"]) == [n] * 3 and list(c["chunks"]) == [-(-n // 1024)] * 3 and list(c["blocks"]) == [n] * 6
                and list(c["segs"]) == [-(-n // 256)] * 6)
    return check


def _switch(n):
    return lambda c, g: c["n_obs"] == n and c["per_cam"].max() > 4096


def _points(n):
    return lambda c, g: (c["n_points"] == n and c["per_point"][n - 1] == 0 and c["per_point"][:n - 1].min() > 0
                         and -(-n // 256) == (1 if n <= 256 else 2))


def _free_extras(fixed):
    def check(c, g):
        pts, cams = bc.unobserved_points(g), bc.unobserved_cams(g)
        return (len(pts) == 5 and len(cams) == 1 and all((g["point_free"][p] == 0) == fixed for p in pts)
                and all(((g["cam_dof"][k] & 63) == 0) == fixed for k in cams))
    return check


def _depth_edge(c, g):
    d = bc.depths(g)[-3:]
    return (d[0] == 0.5e-9 and d[1] == 1e-9 and d[2] == 2e-9 and (bc.depths(g)[:-3] > 0.5).all()
            and list(c["per_point"][-3:]) == [1, 1, 1] and g["cam_dof"][-1] == 0)


def _behind(c, g):
    behind = bc.depths(g) <= 0
    cams = g["obs_cam"][behind]
    return behind.sum() == bc.BEHIND and sorted(set(cams)) == [1, 4] and (cams == 1).sum() == bc.BEHIND // 2 and (bc.depths(g)[~behind] > 0.5).all()


def _info_kinds(c, g):
    L = g["obs_info"].reshape(-1, 2, 2)
    ev = np.linalg.eigvalsh(L)
    sym = np.array_equal(L, L.transpose(0, 2, 1))
    zero = (np.abs(L).max(axis=(1, 2)) == 0)
    rank1 = ~zero & (np.abs(ev[:, 0]) <= 1e-15 * ev[:, 1])
    tiny = g["obs_point"] < bc.TINY_INFO_POINTS
    return (sym and (ev[:, 0] >= -1e-15 * ev[:, 1]).all() and zero.sum() >= 20 and rank1.sum() >= 20 and tiny.sum() >= 10
            and np.array_equal(L[tiny], np.broadcast_to(1e-8 * np.eye(2), L[tiny].shape)))


def _poison(key, row):
    def check(c, g):
        bad = ~np.isfinite(g[key])
        return bad.sum() == 1 and bad[row].sum() == 1 and all(np.isfinite(g[k]).all() for k in ("cam_pose", "point_xyz", "obs_xy") if k != key)
    return check


STRUCTURE = dict(("dense3_%d" % n, _dense3(n)) for n in bc.DENSE3)
STRUCTURE.update(("switch_%d" % n, _switch(n)) for n in (19999, 20000, 20001))
STRUCTURE.update(("points_%d" % n, _points(n)) for n in bc.POINT_EDGES)
STRUCTURE.update({
    "unobserved": _free_extras(False), "unobserved_fixed": _free_extras(True),
    "single_obs_points": lambda c, g: list(c["per_point"][:10]) == [1] * 10 and c["per_point"][10:].min() >= 3,
    "all_cams_fixed": lambda c, g: not (g["cam_dof"] & 63).any() and g.get("point_free") is None,
    "all_points_fixed": lambda c, g: not g["point_free"].any() and ((g["cam_dof"] & 63) != 0).sum() == 5,
    "everything_fixed": lambda c, g: not (g["cam_dof"] & 63).any() and not g["point_free"].any() and c["n_obs"] > 0,
    "gauge_free": lambda c, g: list(g["cam_dof"]) == [63] * 6,
    "one_camera_fixed": lambda c, g: c["n_cams"] == 1 and g["cam_dof"][0] == 0 and list(c["per_point"]) == [1] * 40,
    "one_camera_free_points_fixed": lambda c, g: c["n_cams"] == 1 and g["cam_dof"][0] == 63 and not g["point_free"].any(),
    "two_cams_one_point": lambda c, g: (c["n_cams"], c["n_points"], c["n_obs"]) == (2, 1, 2) and list(c["per_cam"]) == [1, 1],
    "no_points": lambda c, g: (c["n_cams"], c["n_points"], c["n_obs"]) == (4, 0, 0) and g["point_xyz"].shape == (0, 3),
    "no_obs": lambda c, g: c["n_obs"] == 0 and c["n_points"] == 120 and c["n_cams"] == 6,
    "zero_iterations": lambda c, g: bc.CASES["zero_iterations"]["max_iterations"] == 0 and c["n_obs"] == 480,
    "hub_point": lambda c, g: (c["n_cams"] == 130 and c["per_point"][0] == 135 and c["span"] == 129 and (bc.depths(g)[-130:] > 8.0).all()
                               and sorted(g["obs_cam"][-130:]) == list(range(130))),
    "same_camera_twice": lambda c, g: c["per_cam"][1] == 1130 and c["chunks"][1] == 2 and c["pairs"][1, 1] == 1070 + 4 * 30,
    "nonunit_quat": lambda c, g: np.allclose(np.linalg.norm(g["cam_pose"][:, :4], axis=1), [1, 1, 1.3, 1, 0.5, 1], atol=1e-12) and
                                 np.allclose(g["cam_pose"][3, :4], -bc.base()["cam_pose"][3, :4], atol=0) and ((g["cam_dof"][2:5] & 63) == 63).all(),
    "extra_dof_bits": lambda c, g: list(g["cam_dof"]) == [0, 63 | 64, 127, (1 << 20) | 63, 64, 63],
    "dof_masks": lambda c, g: list(g["cam_dof"]) == [0, 56, 7, 62, 63, 63],
    "rank1_and_zero_info": _info_kinds,
    "damping_floor": lambda c, g: bc.CASES["damping_floor"]["max_iterations"] == 2 and _info_kinds(c, g),
    "zero_info": lambda c, g: not g["obs_info"].any() and g["obs_info"].shape == (480, 4),
    "huber_off": lambda c, g: bc.CASES["huber_off"]["huber"] == 0.0,
    "huber_negative": lambda c, g: bc.CASES["huber_negative"]["huber"] < 0,
    "huber_1e300": lambda c, g: bc.CASES["huber_1e300"]["huber"] == 1e300,
    "huber_1e-300": lambda c, g: bc.CASES["huber_1e-300"]["huber"] == 1e-300,
    "depth_edge": _depth_edge, "behind_at_start": _behind,
    "nan_obs": _poison("obs_xy", 37), "inf_obs": _poison("obs_xy", 37), "nan_pose": _poison("cam_pose", 3), "nan_point": _poison("point_xyz", 11)})


def test_every_case_reaches_what_it_is_named_for():
    assert sorted(STRUCTURE) == sorted(bc.NAMES)
    seen = {}
    for name in bc.NAMES:
        g = bc.CASES[name]["graph"]
        c = census(g)
        seen[name] = c
        assert STRUCTURE[name](c, g), name
        print("%-30s cams %3d points %4d obs %5d  obs/cam max %4d (chunks max %d)  pairs/block max %4d (segments max %d)  observers/point %d .. %d" % (
            name, c["n_cams"], c["n_points"], c["n_obs"], c["per_cam"].max(), c["chunks"].max(), c["blocks"].max() if len(c["blocks"]) else 0,
            c["segs"].max() if len(c["segs"]) else 0, c["per_point"].min() if c["n_points"] else 0, c["per_point"].max() if c["n_points"] else 0))
    # what the census as a whole must contain
    chunks = set(int(v) for c in seen.values() for v in c["chunks"])
    assert {0, 1, 2, 3, 5} <= chunks
    per_cam = set(int(v) for c in seen.values() for v in c["per_cam"])
    assert {1023, 1024, 1025} <= per_cam      # 1 chunk, exactly 1 chunk, 2 chunks
    blocks = set(int(v) for c in seen.values() for v in c["blocks"])
    assert {255, 256, 257, 1023, 1024, 1025} <= blocks
    assert {19999, 20000, 20001} <= set(c["n_obs"] for c in seen.values())
    assert set(int(v) for v in seen["dense3_1025"]["segs"]) == {5} and set(int(v) for v in seen["dense3_1024"]["segs"]) == {4}
    assert set(int(v) for v in seen["dense3_1024"]["chunks"]) == {1} and set(int(v) for v in seen["dense3_1025"]["chunks"]) == {2}


# ------------------------------------------------------------------------------------------------ oracle runs
@pytest.fixture(scope="module")
def runs(oracle):
    return dict((name, oracle.ba_solve(bc.CASES[name]["graph"], _opts(bc.CASES[name]))) for name in bc.NAMES)


def _same_state(got, g):
    return got[0].tobytes() == np.ascontiguousarray(g["cam_pose"], np.float64).tobytes() and got[1].tobytes() == np.ascontiguousarray(g["point_xyz"], np.float64).tobytes()


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_on_the_census(runs, name):
    g = bc.CASES[name]["graph"]
    poses, pts, sm, st = runs[name]
    trace = [sm.trace_cost[i] for i in range(sm.trace_len)]
    print("%s: status %d, %d iterations (%d accepted), termination %d, cost %.6e -> %.6e" % (name, st, sm.iterations, sm.accepted, sm.termination,
                                                                                            sm.initial_cost, sm.final_cost))
    for c in bc.fixed_cams(g) + bc.unobserved_cams(g) * (name == "unobserved_fixed"):
        assert poses[c].tobytes() == g["cam_pose"][c].tobytes(), c
    for p in bc.fixed_points(g):
        assert pts[p].tobytes() == g["point_xyz"][p].tobytes(), p
    for p in bc.unobserved_points(g):  # no gradient: the damped step of an unobserved point is exactly zero
        assert pts[p].tobytes() == g["point_xyz"][p].tobytes(), p
    if name in bc.NOTHING_TO_DO:
        assert st == 0 and (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (0, 0, 2, 0) and _same_state((poses, pts), g)
        assert sm.final_cost == sm.initial_cost
    elif name == "zero_iterations":
        assert st == 0 and (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (0, 0, 0, 0) and _same_state((poses, pts), g)
    elif name in ("nan_obs", "inf_obs"):
        assert st == 1 and (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (15, 0, 3, 15)
        assert np.isnan(sm.initial_cost) and all(np.isinf(v) and v > 0 for v in trace) and _same_state((poses, pts), g)
    else:
        assert st == 0 and sm.final_cost < sm.initial_cost and sm.accepted >= 1 and np.isfinite(sm.initial_cost)
        if name == "nan_pose":
            assert np.isnan(poses[3]).any() and np.isfinite(np.delete(poses, 3, axis=0)).all() and np.isfinite(pts).all()
        elif name == "nan_point":
            assert np.isnan(pts[11]).any() and np.isfinite(np.delete(pts, 11, axis=0)).all() and np.isfinite(poses).all()
        else:
            assert np.isfinite(poses).all() and np.isfinite(pts).all()
    if name == "dof_masks":  # a masked translation stays bit for bit; a masked rotation is renormalised and nothing more
        assert poses[1, 4:].tobytes() == g["cam_pose"][1, 4:].tobytes() and poses[1, :4].tobytes() != g["cam_pose"][1, :4].tobytes()
        assert np.abs(poses[2, :4] - g["cam_pose"][2, :4]).max() <= 4e-16 and poses[2, 4:].tobytes() != g["cam_pose"][2, 4:].tobytes()
    if name == "depth_edge":  # at and below kMinDepth the observation does not exist; the points it alone sees stay put
        n = len(pts)
        assert pts[n - 3].tobytes() == g["point_xyz"][n - 3].tobytes() and pts[n - 2].tobytes() == g["point_xyz"][n - 2].tobytes()
        assert pts[n - 1].tobytes() != g["point_xyz"][n - 1].tobytes()


def test_gate_classes_agree_with_their_twins(runs):
    """Huber off, negative and huge are the same problem, bit for bit; extras that nothing observes change nothing."""
    a = runs["huber_off"]
    for other in ("huber_negative", "huber_1e300"):
        b = runs[other]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].final_cost == b[2].final_cost
    a, b = runs["unobserved"], runs["unobserved_fixed"]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------ linearisation
def _lin(oracle, pose, dof, X, pfree, m, info=None, huber=0.01):
    r, Jc, Jp = np.zeros(2), np.zeros(12), np.zeros(6)
    w, s = C.c_double(), C.c_double()
    hold = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (pose, X, m, info)]
    q = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ok = oracle.lib.oracle_ba_obs_linearize(q(hold[0]), int(dof), q(hold[1]), int(pfree), q(hold[2]), q(hold[3]), C.c_double(huber),
                                            q(r), C.byref(w), q(Jc), q(Jp), C.byref(s))
    return ok, r, w.value, Jc.reshape(2, 6), Jp.reshape(2, 3), s.value


def _mp_lin(mp, pose, X, m, info, huber):
    """-> (in front, r 2, w, Jc 2 x 6, Jp 2 x 3) in mpmath; see the module docstring."""
    f = lambda v: mp.mpf(float(v))
    x, y, z, w = [f(v) for v in pose[:4]]
    K = mp.matrix([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    M = mp.eye(3) + 2 * w * K + 2 * (K * K)
    Xc0 = M.T * mp.matrix([f(X[i]) - f(pose[4 + i]) for i in range(3)])
    if not Xc0[2] > f(bc.MIN_DEPTH):
        return False, None, None, None, None

    def res(v):
        G = mp.matrix(4, 4)
        G[0, 1], G[0, 2], G[1, 0], G[1, 2], G[2, 0], G[2, 1] = -v[5], v[4], v[5], -v[3], -v[4], v[3]
        G[0, 3], G[1, 3], G[2, 3] = v[0], v[1], v[2]
        E = mp.expm(G) if any(G) else mp.eye(4)
        Xw = Xc0 + M.T * mp.matrix(v[6:9])
        Xc = E[:3, :3].T * (Xw - E[:3, 3])
        return [Xc[0] / Xc[2] - f(m[0]), Xc[1] / Xc[2] - f(m[1])]

    zero = [mp.mpf(0)] * 9
    r = res(zero)
    h = mp.mpf(10) ** -20
    J = np.zeros((2, 9))
    for k in range(9):
        up, dn = list(zero), list(zero)
        up[k], dn[k] = h, -h
        a, b = res(up), res(dn)
        J[:, k] = [float((a[e] - b[e]) / (2 * h)) for e in range(2)]
    L = [[mp.mpf(1), mp.mpf(0)], [mp.mpf(0), mp.mpf(1)]] if info is None else [[f(info[0]), f(info[1])], [f(info[2]), f(info[3])]]
    s = r[0] * (L[0][0] * r[0] + L[0][1] * r[1]) + r[1] * (L[1][0] * r[0] + L[1][1] * r[1])
    d = f(huber)
    wgt = d / mp.sqrt(s) if d > 0 and s > d * d else mp.mpf(1)
    return True, np.array([float(r[0]), float(r[1])]), float(wgt), J[:, :6], J[:, 6:]


def _lin_inputs():
    """[(class, pose, X, m, info, huber)]"""
    out = []
    g = bc.CASES["unobserved"]["graph"]
    for k in range(0, 480, 8):
        out.append(("base", g["cam_pose"][g["obs_cam"][k]], g["point_xyz"][g["obs_point"][k]], g["obs_xy"][k], None, 0.01))
    g = bc.CASES["depth_edge"]["graph"]
    for k in (-3, -2, -1):
        out.append(("depth_edge", g["cam_pose"][g["obs_cam"][k]], g["point_xyz"][g["obs_point"][k]], g["obs_xy"][k], None, 0.01))
    g = bc.CASES["nonunit_quat"]["graph"]
    for k in np.flatnonzero(np.isin(g["obs_cam"], (2, 3, 4)))[::6]:
        out.append(("nonunit_quat", g["cam_pose"][g["obs_cam"][k]], g["point_xyz"][g["obs_point"][k]], g["obs_xy"][k], None, 0.01))
    g = bc.CASES["rank1_and_zero_info"]["graph"]
    L = g["obs_info"].reshape(-1, 2, 2)
    singular = np.flatnonzero(np.abs(np.linalg.det(L)) <= 1e-15 * np.abs(L).max(axis=(1, 2)) ** 2)
    for k in singular[::4]:
        out.append(("rank1_info", g["cam_pose"][g["obs_cam"][k]], g["point_xyz"][g["obs_point"][k]], g["obs_xy"][k], g["obs_info"][k], 0.01))
    # a residual of exactly (delta, 0): the identity pose and a point on the axis, u = v = 0 exactly, m = (-delta, 0)
    delta = 0.01
    for d in (np.nextafter(delta, 0), delta, np.nextafter(delta, 1)):
        out.append(("huber_edge", np.array([0, 0, 0, 1.0, 0, 0, 0]), np.array([0, 0, 2.0]), np.array([-d, 0.0]), None, delta))
    return out


def test_linearisation_against_mpmath(oracle):
    import mpmath as mp
    worst, invalid, weights = {}, {}, []
    with mp.workdps(50):
        for cls, pose, X, m, info, huber in _lin_inputs():
            ok, r, w, Jc, Jp, s = _lin(oracle, pose, 63, X, 1, m, info, huber)
            front, r_ref, w_ref, Jc_ref, Jp_ref = _mp_lin(mp, pose, X, m, info, huber)
            assert bool(ok) == front, (cls, pose, X)
            if not front:
                invalid[cls] = invalid.get(cls, 0) + 1
                continue
            err = max([ULP] + [np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in ((r, r_ref), (Jc, Jc_ref), (Jp, Jp_ref), (np.array([w]), np.array([w_ref])))])
            worst[cls] = max(worst.get(cls, 0.0), err)
            assert err <= LIN_BAR[cls], (cls, err)
            if cls == "huber_edge":
                weights.append((s, w))
    print("worst linearisation error per class:", dict((k, "%.1e" % v) for k, v in sorted(worst.items())))
    print("observations that do not exist (depth <= 1e-9) on both sides, per class:", invalid)
    assert sorted(worst) == sorted(LIN_BAR) and invalid["depth_edge"] == 2  # depths 0.5e-9 and exactly 1e-9 do not exist
    d2 = 0.01 * 0.01
    assert [s > d2 for s, _ in weights] == [False, False, True] and weights[1][0] == d2
    assert weights[0][1] == 1.0 and weights[1][1] == 1.0 and weights[2][1] < 1.0  # s == delta^2 is still quadratic


# ------------------------------------------------------------------------------------------------ first LM step, dense
def _solve_spd_longdouble(A, b):
    """Gaussian elimination without pivoting (A is symmetric positive definite) in longdouble."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


@pytest.mark.parametrize("name", sorted(STEP_BAR))
def test_first_lm_step_without_schur(oracle, name):
    case = bc.CASES[name]
    g, huber, radius = case["graph"], case["huber"], np.longdouble(1e4)
    nc, npnt, no = len(g["cam_dof"]), len(g["point_xyz"]), len(g["obs_cam"])
    pfree = g.get("point_free")
    col, ncol = {}, 0
    for c in range(nc):
        for k in range(6):
            if (int(g["cam_dof"][c]) >> k) & 1:
                col[("c", c, k)] = ncol
                ncol += 1
    for p in range(npnt):
        if pfree is None or pfree[p]:
            for k in range(3):
                col[("p", p, k)] = ncol
                ncol += 1
    H, grad = np.zeros((ncol, ncol), np.longdouble), np.zeros(ncol, np.longdouble)
    for k in range(no):
        c, p = int(g["obs_cam"][k]), int(g["obs_point"][k])
        info = g["obs_info"][k] if "obs_info" in g else None
        ok, r, w, Jc, Jp, s = _lin(oracle, g["cam_pose"][c], int(g["cam_dof"][c]), g["point_xyz"][p], 1 if pfree is None else int(pfree[p]),
                                   g["obs_xy"][k], info, huber)
        if not ok:
            continue
        idx = [col[("c", c, a)] for a in range(6) if ("c", c, a) in col] + [col[("p", p, a)] for a in range(3) if ("p", p, a) in col]
        J = np.concatenate([Jc[:, [a for a in range(6) if ("c", c, a) in col]], Jp[:, [a for a in range(3) if ("p", p, a) in col]]], axis=1).astype(np.longdouble)
        L = np.longdouble(w) * (np.eye(2) if info is None else info.reshape(2, 2)).astype(np.longdouble)
        H[np.ix_(idx, idx)] += J.T @ L @ J
        grad[idx] += J.T @ (L @ r.astype(np.longdouble))
    diag = np.diag(H).copy()
    # what each case brings to the damping: columns of zeros, diagonals under the 1e-6 floor, a rank-2 point block, points only
    if name == "unobserved":
        assert (diag == 0).sum() == 6 + 3 * 5
    elif name == "rank1_and_zero_info":
        assert ((diag > 0) & (diag < 1e-6)).sum() >= 3 * bc.TINY_INFO_POINTS
    elif name == "single_obs_points":
        for p in range(10):
            ev = np.linalg.eigvalsh(H[np.ix_(*[[col[("p", p, a)] for a in range(3)]] * 2)].astype(np.float64))
            assert abs(ev[0]) <= 1e-12 * ev[2] and ev[1] > 1e-6 * ev[2]
    else:
        assert ncol == 3 * npnt
    H[np.diag_indices(ncol)] += np.clip(diag, np.longdouble(1e-6), np.longdouble(1e32)) / radius
    step = _solve_spd_longdouble(H, -grad).astype(np.float64)
    poses, pts = g["cam_pose"].copy(), g["point_xyz"].copy()
    for c in range(nc):
        if int(g["cam_dof"][c]) & 63:
            xi = np.array([step[col[("c", c, a)]] if ("c", c, a) in col else 0.0 for a in range(6)])
            poses[c] = oracle.se3_retract(g["cam_pose"][c], xi)
    for (kind, p, a), j in col.items():
        if kind == "p":
            pts[p, a] += step[j]
    mine = oracle.ba_cost(g, poses, pts, huber=huber)
    _, _, sm, st = oracle.ba_solve(g, _opts(case, 1))
    assert st == 0 and sm.trace_len == 1 and sm.trace_accepted[0] == 1
    rel = max(abs(mine - sm.trace_cost[0]) / sm.trace_cost[0], ULP)  # (a float64 cost cannot be compared finer than its last bit)
    print("%s: first candidate %.17g, dense longdouble step %.17g, relative difference %.1e" % (name, sm.trace_cost[0], mine, rel))
    assert rel <= STEP_BAR[name]


# ------------------------------------------------------------------------------------------------ yardstick
def measure_yardstick(oracle, fma, name):
    case = bc.CASES[name]
    a, b = oracle.ba_solve(case["graph"], _opts(case)), fma.ba_solve(case["graph"], _opts(case))
    sa, sb = a[2], b[2]
    assert (a[3], sa.iterations, sa.accepted, sa.termination, sa.trace_len) == (b[3], sb.iterations, sb.accepted, sb.termination, sb.trace_len), name
    assert [sa.trace_accepted[i] for i in range(sa.trace_len)] == [sb.trace_accepted[i] for i in range(sb.trace_len)], name
    return max([float(np.abs(a[k] - b[k]).max()) for k in (0, 1) if a[k].size])


def test_yardstick(oracle):
    fma = oracle_lib.Oracle(os.path.join(oracle_lib.ROOT, "oracle", "liboracle_fma.so"))
    assert sorted(bc.YARDSTICK) == sorted(bc.FINITE)
    for name in bc.FINITE:
        got, rec = measure_yardstick(oracle, fma, name), bc.YARDSTICK[name]
        print("    %-32s %.2e (recorded %.2e)" % ('"%s":' % name, got, rec))
        assert (got == 0.0 and rec == 0.0) or (0.5 * rec <= got <= 2.0 * rec), (name, got, rec)
    structural = [n for n in bc.FINITE if n.startswith(("dense3_", "switch_", "points_"))]
    assert max(bc.YARDSTICK[n] for n in structural) <= 1e-12


# ------------------------------------------------------------------------------------------------ pose-only LM
def test_pnp_oracle_on_its_edges(oracle):
    for name, (X, m, pose, dof) in bc.PNP_CASES.items():
        p, sm, _, rc = oracle.ba_pnp(X, m, pose, dof=dof, opts=oracle_lib.ba_options(max_iterations=20))
        print("pnp %s: status %d, %d iterations, termination %d, cost %.3e -> %.3e" % (name, rc, sm.iterations, sm.termination, sm.initial_cost, sm.final_cost))
        assert rc == 0 and np.isfinite(p).all()
        if name in bc.PNP_NOTHING_TO_DO:
            assert (sm.iterations, sm.termination) == (0, 2) and p.tobytes() == np.asarray(pose, np.float64).tobytes()
        else:
            assert sm.final_cost < sm.initial_cost
        if dof == 7:
            assert np.abs(p[:4] - pose[:4]).max() <= 4e-16  # translation only: the rotation is renormalised, nothing more
