"""gh_graph_solve WITH landmarks (the gr_* kernels of gslam_amd/csrc/posegraph.hip: XYZ and inverse-depth points, the sphere
projection, camera self-calibration) on the census of tests/graph_adversarial_cases.py, against oracle/graph_oracle.c.  The
oracle itself is pinned to independent references in tests/test_graph_adversarial_oracle.py.

Bars (those of tests/test_graph_gpu.py and tests/test_calib_gpu.py, unchanged): status 0 on both sides, initial cost 1e-12,
identical iteration count / accepted count / termination / trace length and the same accept / reject at every iteration,
`inf` candidate costs in the same places, every cost of the trace and the final cost to 1e-9 (+ 1e-15 absolute), frames
1e-8, landmarks 1e-7, inverse depths 1e-8 relative (+ 1e-10), intrinsics 1e-8 (focal lengths and principal point relative,
distortion absolute).  A case's state bars are max(that bar, 8 x its yardstick state figure), its cost bar
max(1e-9, 8 x its yardstick cost figure) -- graph_adversarial_cases.YARDSTICK, how far FMA contraction alone moves the
oracle; 8 is the room a different summation order gets over a different rounding.  No yardstick figure reaches an eighth
of a state bar (the largest: cam_underdetermined 1.2e-9, info_rank1_zero_scales 4.3e-10), so every state bar is the existing
one.  Seven cost bars are wider than 1e-9: obs_16 5.4e-9, obs_17 4.4e-9, cam_obs_63 / 64 / 65 4.1e-9 / 6.5e-9 / 4.8e-9,
no_obs_pose_edges 2.1e-8, cam_underdetermined 5.3e-8.

Every finite case runs twice in the reproducible mode (gh_ba_options.deterministic = 1, the default): frames, points, inverse
depths, intrinsics and every cost of the trace bit for bit the same.  BOTH_MODES (hub, duplicates, boundaries, camera) run
with deterministic = 0 as well, compared with lm_trace.assert_same_trace.  Fixed frames, fixed landmarks, landmarks nothing
(valid) observes and fixed intrinsics come back bit for bit.  Twins are compared GPU against GPU at the bars.

Which kernels run is read off the profile: gr_schur_cam / gr_schur_cam_cc / gr_cam_fold with free intrinsics and never
without; gr_lm_sum and gr_det_fold in the reproducible mode only; no gr_* kernel that works on observations when there are
none.  With every landmark fixed gr_schur is still launched (the launch depends on the counts alone) and every thread leaves
at lmdim == 0: that it adds nothing is what the parity of all_landmarks_fixed shows, the oracle's Schur loop skips dp == 0.

Non-finite cases.  No device-side wait of a solve depends on a value a NaN can reach (read off the code, not probed):
  - the LM loop of gh_graph_solve runs max_iterations times at the most and launches the same kernels whatever the data
    holds; every loop of a gr_* kernel runs over lstart / llist ranges or fixed counts (gr_cam_fold's `while` walks the
    54 words of the intrinsics triangle by thread index);
  - acc_add adds a NaN like any other number; the bound of the reproducible accumulation takes `B > 0 && B < 1e300`,
    which a NaN or an inf fails: the quantum then comes from the other observations;
  - the gradient maximum goes through `v > 0` and atomicMax on the bits, which drop a NaN (the oracle's fmax does too);
  - the dense solve is gh_potrf_solve_dev, the single-launch factorisation and back-substitution of the bundle adjustment:
    its waits poll arrival counters that every publishing wave increments, bad pivot or not, each bounded by a spin limit
    with a common abort word (chol.hip; tests/test_ba_adversarial_gpu.py lists them).
So the four cases run here, once each, with three iterations.

What the census found.  The reproducible accumulation used ONE bound for every word of the reduced system, so a single
observation with large Jacobians set the quantum of blocks it does not add to: depth_edge (a point 2e-9 in front of a FIXED
camera: d r / d X of 5e8) solved in 13 iterations with the first candidate's cost 4.4e-3 off and the frames 2.6e-3, where the
oracle and deterministic = 0 take 4; sim3_scales (keyframe scales 1e-3 and 1e3) had the first candidate's cost 8.2e-9 off and
the frames 3.1e-7.  Fixed in posegraph.hip (DetAcc: one bound per keyframe block, the landmark's own Jacobian in none of
them); DESIGN.md has the argument.  Nothing else disagreed.

Measured on an MI355X (GSLAM_TEST_PRINT_DIFFS=1 prints every case), worst per class, GPU against oracle -- frames / landmarks /
intrinsics / costs beyond 1e-15 (inverse depths: nothing beyond the 1e-10 absolute anywhere):
    structure (base, shuffled, relabelled, duplicates, lone, unobserved, fixed, host groups, hubs, one / two frames)
                                        2.4e-14 / 1.6e-13 (lone_xyz) / - / 0       frame_without_obs 1.5e-11 / 9.7e-12
    landmark boundaries lm_255 .. 257   8.9e-15 / 1.1e-14 / - / 0
    observation boundaries obs_15 .. 17 1.0e-12 / 3.5e-12 / - / 1.4e-10
    camera boundaries cam_obs_1 .. 129  1.8e-12 / 1.6e-11 / 9.2e-14 / 1.4e-9 (cam_obs_63: bar 4.1e-9), cam_waves_18 3.7e-15 / 5.3e-15 / 2.2e-16 / 1.7e-14
    depth_edge, behind_*, step_pushes_behind, rho_floor, huber_*, far_world, sphere cases
                                        9.8e-15 / 1.2e-14 / - / 0
    rho_huge 5.4e-13 / 2.4e-13 / - / 2.2e-13     sim3_scales 1.3e-10 / 5.4e-12 / - / 0     info_rank1_zero_scales 3.8e-10 / 2.0e-10 / - / 8.8e-12
    cam_fixed_pixels, cam_fold_over     1.5e-14 / 7.1e-15 / 6.6e-16 / 3.6e-14        cam_unobservable 4.8e-14 / 2.0e-13 / 1.2e-9 / 4.4e-13
    cam_underdetermined                 6.0e-10 / 2.2e-10 / 4.6e-11 / 1.5e-8 (bar 5.3e-8)
    no_obs_pose_edges                   5.4e-12 / 0 / - / 0 (bar 2.1e-8)
    twins GPU against GPU               3.6e-15 / 7.1e-15; relabelled landmarks, unobserved landmarks and the invalid first observation: 0 (bit for bit)
    deterministic = 0 (BOTH_MODES)      identical decisions everywhere; 5.9e-12 / 8.0e-12 / 3.1e-15
The 88 tests of this file take 3.2 s together (0.03 s the slowest, after 1.7 s for the context)."""
import ctypes as C
import os

import numpy as np
import pytest

import graph_adversarial_cases as gc
from lm_trace import assert_same_trace
from test_graph_adversarial_oracle import accepts, costs, same_state, solve as oracle_solve, untouched

pytestmark = pytest.mark.gpu

INITIAL_RTOL, COST_RTOL, COST_ATOL = 1e-12, 1e-9, 1e-15
FRAMES, LANDMARKS, RHO_RTOL, RHO_ATOL, INTRINSICS = 1e-8, 1e-7, 1e-8, 1e-10, 1e-8


def bars(*names):
    """(frames, landmarks, rho relative, intrinsics, cost) for a comparison that involves these cases."""
    y = max(gc.YARDSTICK.get(n, (0.0, 0.0))[0] for n in names)
    c = max(gc.YARDSTICK.get(n, (0.0, 0.0))[1] for n in names)
    return max(FRAMES, 8 * y), max(LANDMARKS, 8 * y), max(RHO_RTOL, 8 * y), max(INTRINSICS, 8 * y), max(COST_RTOL, 8 * c)


def gpu_solve(ctx, case, deterministic=1):
    from gslam_amd import ba, posegraph
    opts = ba.default_options(huber_delta=case["huber"], max_iterations=case["max_iterations"], deterministic=deterministic)
    out = posegraph.solve_graph(ctx, case["start"], case["dof"], case["problem"], opts)
    if case["problem"].get("intrinsics") is not None:
        S, xyz, rho, cam, sm, st = out
    else:
        (S, xyz, rho, sm, st), cam = out, None
    return {"S": S, "xyz": xyz, "rho": rho, "cam": cam, "sm": sm, "st": st}


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """The oracle's solve of every case, once."""
    return dict((name, oracle_solve(oracle, gc.CASES[name])) for name in gc.NAMES)


def _close(a, b, rtol, atol=0.0):
    return abs(a - b) <= rtol * abs(b) + atol


def same_trace(sg, so, name, cost_rtol):
    assert (sg.iterations, sg.accepted, sg.termination, sg.trace_len) == (so.iterations, so.accepted, so.termination, so.trace_len), name
    assert accepts(sg) == accepts(so), (name, accepts(sg), accepts(so))
    worst = 0.0
    for i, (cg, co) in enumerate(zip(costs(sg), costs(so))):
        if not np.isfinite(co):
            assert cg == co or (np.isnan(cg) and np.isnan(co)), (name, i, cg, co)
        else:
            worst = max(worst, max(abs(cg - co) - COST_ATOL, 0.0) / abs(co) if co else 0.0)
            assert _close(cg, co, cost_rtol, COST_ATOL), (name, "cost at iteration %d" % i, cg, co)
    return worst


def state_differences(a, b, twin=None):
    """(frames, landmarks, rho relative beyond RHO_ATOL, intrinsics); twin: index arrays that put a's blocks into b's order."""
    twin = twin or {}
    pick = lambda arr, key: arr if twin.get(key) is None else arr[twin[key]]
    ok = lambda x: np.where(np.isfinite(x), x, 0.0)
    S, xyz, rho = pick(a["S"], "frames"), pick(a["xyz"], "xyz"), pick(a["rho"], "idp")
    dS = float(np.abs(ok(S - b["S"])).max())
    dX = float(np.abs(ok(xyz - b["xyz"])).max()) if b["xyz"].size else 0.0
    dR = float((np.maximum(np.abs(rho - b["rho"]) - RHO_ATOL, 0.0) / np.abs(b["rho"])).max()) if b["rho"].size else 0.0
    dC = 0.0
    if b["cam"] is not None:
        dC = max(float((np.abs(a["cam"][:4] - b["cam"][:4]) / np.abs(b["cam"][:4])).max()), float(np.abs(a["cam"][4:] - b["cam"][4:]).max()))
    return dS, dX, dR, dC


def compare(got, ref, name, others=(), twin=None, what="oracle"):
    case = gc.CASES[name]
    bf, bl, br, bc, bcost = bars(name, *others)
    sg, so = got["sm"], ref["sm"]
    dS, dX, dR, dC = state_differences(got, ref, twin)
    if os.environ.get("GSLAM_TEST_PRINT_DIFFS"):  # every figure before anything is asserted
        worst = max([0.0] + [max(abs(cg - co) - COST_ATOL, 0.0) / abs(co) for cg, co in zip([sg.initial_cost, sg.final_cost] + costs(sg), [so.initial_cost, so.final_cost] + costs(so))
                             if np.isfinite(co) and np.isfinite(cg) and co != 0.0])
        print("DIFF %s against %s: frames %.2e (bar %.1e) landmarks %.2e (%.1e) rho %.2e (%.1e) intrinsics %.2e (%.1e) costs %.2e (%.1e) decisions %s / %s" % (
            name, what, dS, bf, dX, bl, dR, br, dC, bc, worst, bcost, "".join(map(str, accepts(sg))), "".join(map(str, accepts(so)))))
    assert got["st"] == ref["st"] == 0, name
    assert _close(sg.initial_cost, so.initial_cost, INITIAL_RTOL, COST_ATOL), (name, sg.initial_cost, so.initial_cost)
    same_trace(sg, so, name, bcost)
    assert _close(sg.final_cost, so.final_cost, bcost, COST_ATOL), name
    assert dS <= bf and dX <= bl and dR <= br and dC <= bc, (name, dS, dX, dR, dC)
    if twin is None:
        untouched(got, case, name)
        if name in gc.NOTHING_TO_DO:
            assert (sg.iterations, sg.accepted, sg.termination, sg.trace_len) == (0, 0, 2, 0) and same_state(got, case) and sg.final_cost == sg.initial_cost


def same_bits(a, b):
    sa, sb = a["sm"], b["sm"]
    return (a["st"] == b["st"] and a["S"].tobytes() == b["S"].tobytes() and a["xyz"].tobytes() == b["xyz"].tobytes() and a["rho"].tobytes() == b["rho"].tobytes()
            and (a["cam"] is None) == (b["cam"] is None) and (a["cam"] is None or a["cam"].tobytes() == b["cam"].tobytes())
            and (sa.iterations, sa.accepted, sa.termination, sa.trace_len) == (sb.iterations, sb.accepted, sb.termination, sb.trace_len)
            and np.array([sa.initial_cost, sa.final_cost] + costs(sa)).tobytes() == np.array([sb.initial_cost, sb.final_cost] + costs(sb)).tobytes()
            and accepts(sa) == accepts(sb))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", gc.FINITE)
def test_census_against_the_oracle(ctx, oracle_runs, name):
    case = gc.CASES[name]
    a, b = gpu_solve(ctx, case), gpu_solve(ctx, case)
    assert same_bits(a, b), (name, "gh_graph_solve is not reproducible run to run")
    compare(a, oracle_runs[name], name)


@pytest.mark.parametrize("name", gc.BOTH_MODES)
def test_plain_atomics_still_agree(ctx, oracle_runs, name):
    """deterministic = 0: the same run up to the settled tail (lm_trace.assert_same_trace); where the decisions are the
    same all the way, the states at the bars."""
    got, ref = gpu_solve(ctx, gc.CASES[name], deterministic=0), oracle_runs[name]
    assert got["st"] == ref["st"] == 0
    if assert_same_trace(got["sm"], ref["sm"], 1e-7):
        bf, bl, br, bc, _ = bars(name)
        dS, dX, dR, dC = state_differences(got, ref)
        if os.environ.get("GSLAM_TEST_PRINT_DIFFS"):
            print("DIFF %s plain atomics: frames %.2e landmarks %.2e rho %.2e intrinsics %.2e" % (name, dS, dX, dR, dC))
        assert dS <= bf and dX <= bl and dR <= br and dC <= bc, (name, dS, dX, dR, dC)
    untouched(got, gc.CASES[name], name)


@pytest.mark.parametrize("name", sorted(gc.TWINS))
def test_twins_gpu_against_gpu(ctx, name):
    """The same problem written differently (a shuffled observation list, relabelled landmarks or frames, every observation
    twice against twice the information, additions that nothing couples to the graph), mapped back."""
    twin = gc.TWINS[name]
    compare(gpu_solve(ctx, gc.CASES[name]), gpu_solve(ctx, gc.CASES[twin["of"]]), name, others=(twin["of"],), twin=twin, what=twin["of"] + " on the GPU")


# ------------------------------------------------------------------------------------------------ which kernels run
def _profiled(ctx, fn):
    ctx.prof_enable(True)
    try:
        out = fn()
        names = set(ctx.prof_collect().keys())
    finally:
        ctx.prof_enable(False)
    return out, names


CAM_KERNELS = {"gr_schur_cam", "gr_schur_cam_cc", "gr_cam_fold"}
DET_KERNELS = {"gr_lm_sum", "gr_det_fold"}
OBS_KERNELS = {"gr_obs_lin", "gr_frame_rows", "gr_schur", "gr_cost"}


def test_the_kernels_a_case_is_aimed_at_run(ctx):
    _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES["cam_obs_65"]))
    assert CAM_KERNELS | DET_KERNELS | OBS_KERNELS | {"gr_lm_prepare", "gr_backsub", "gr_model", "gr_update"} <= k, k
    _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES["cam_obs_65"], deterministic=0))
    assert CAM_KERNELS <= k and not (DET_KERNELS & k), k
    _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES["cam_fixed_pixels"]))   # (given intrinsics are a block of the system, free or not)
    assert CAM_KERNELS <= k, k
    for name in ("dup_same_frame", "all_landmarks_fixed", "lone_xyz"):
        _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES[name]))
        assert OBS_KERNELS | DET_KERNELS <= k and not (CAM_KERNELS & k), (name, k)
    _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES["no_obs_pose_edges"]))
    assert not ((OBS_KERNELS | CAM_KERNELS | DET_KERNELS) & k) and {"pg_edge", "pg_assemble", "gr_lm_prepare", "gr_backsub"} <= k, k
    _, k = _profiled(ctx, lambda: gpu_solve(ctx, gc.CASES["everything_fixed"]))
    assert "gr_obs_lin" in k and "gr_cost" in k   # the gate is taken on a linearisation, not before it


# ------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("name", gc.NON_FINITE)
def test_non_finite_input(ctx, oracle_runs, name):
    case, ref = gc.CASES[name], oracle_runs[name]
    got = gpu_solve(ctx, case)
    sg, so = got["sm"], ref["sm"]
    print("%s: status %d, %d iterations, termination %d, initial cost %r, candidate costs %r" % (name, got["st"], sg.iterations, sg.termination, sg.initial_cost, costs(sg)))
    assert got["st"] == ref["st"] == 0
    same_trace(sg, so, name, COST_RTOL)
    if name in ("nan_obs", "inf_obs"):
        assert np.isnan(sg.initial_cost) and np.isnan(so.initial_cost) and np.isnan(sg.final_cost) and (sg.iterations, sg.accepted, sg.termination) == (3, 0, 0)
        assert all(v == np.inf for v in costs(sg)) and same_state(got, case)
    else:
        assert _close(sg.initial_cost, so.initial_cost, INITIAL_RTOL) and _close(sg.final_cost, so.final_cost, COST_RTOL)
        for key in ("S", "xyz", "rho"):
            assert np.array_equal(np.isfinite(got[key]), np.isfinite(ref[key])), (name, key)
        dS, dX, dR, _ = state_differences(got, ref)
        assert dS <= FRAMES and dX <= LANDMARKS and dR <= RHO_RTOL, (name, dS, dX, dR)
        untouched(got, case, name)
    # the context is as good as before
    compare(gpu_solve(ctx, gc.CASES["two_frames"]), oracle_runs["two_frames"], "two_frames")


# ------------------------------------------------------------------------------------------------ refusals
def _raw_solve(ctx, mutate, sphere=False, with_cam=True):
    """gh_graph_solve through the C ABI on the base graph with DIRTY in / out arrays (valid where the checks read them: scales,
    inverse depths and focal lengths of 7.25) after mutate(arrays, counts, null).  -> (status, untouched, kernels launched)"""
    from gslam_amd import ba, hip
    case = gc.CASES["base"]
    pr = case["problem"]
    kind, point, frame, xy, _ = pr["obs"]
    a = {"S": np.full((6, 8), 7.25), "dof": case["dof"].copy(), "xyz": np.full((20, 3), -3.5), "host": pr["idp"][0].astype(np.int32).copy(),
         "anchor": np.ascontiguousarray(pr["idp"][1], np.float64), "rho": np.full(20, 7.25), "kind": kind.copy(), "point": point.copy(), "frame": frame.copy(),
         "xy": np.ascontiguousarray(np.concatenate([xy, np.ones((len(xy), 1))], axis=1) if sphere else xy), "cam": np.full(9, 7.25)}
    n = {"frames": 6, "xyz": 20, "idp": 20, "obs": len(kind), "cam_free": 3}
    null = set()
    mutate(a, n, null)
    before = dict((k, a[k].tobytes()) for k in ("S", "xyz", "rho", "cam"))
    p = lambda k: None if k in null else a[k].ctypes.data_as(C.c_void_p)
    gp = hip.GraphProblem()
    gp.pg.n_frames, gp.pg.frame_sim3, gp.pg.frame_dof = n["frames"], p("S"), p("dof")
    gp.n_xyz, gp.xyz, gp.xyz_free = n["xyz"], p("xyz"), None
    gp.n_idp, gp.idp_host, gp.idp_anchor, gp.idp_rho, gp.idp_free = n["idp"], p("host"), p("anchor"), p("rho"), None
    gp.n_obs, gp.obs_kind, gp.obs_point, gp.obs_frame, gp.obs_info = n["obs"], p("kind"), p("point"), p("frame"), None
    gp.projection, gp.obs_xy, gp.obs_bearing = (1, None, p("xy")) if sphere else (0, p("xy"), None)
    if with_cam:
        gp.intrinsics, gp.intrinsics_free = p("cam"), n["cam_free"]
    sm = hip.BaSummary()
    opts = ba.default_options(huber_delta=0.01, max_iterations=3)
    st, launched = _profiled(ctx, lambda: hip.lib.gh_graph_solve(ctx.h, C.byref(gp), C.byref(opts), C.byref(sm)))
    return st, all(a[k].tobytes() == before[k] for k in before), launched


def _set(key, index, value):
    def mutate(a, n, null):
        a[key][index] = value
    return mutate


def _count(key, value):
    def mutate(a, n, null):
        n[key] = value
    return mutate


def _null(key):
    return lambda a, n, null: null.add(key)


def test_bad_problems_are_refused_and_left_untouched(ctx, oracle_runs):
    bad = {"obs_frame = n_frames": _set("frame", 77, 6), "obs_frame = -1": _set("frame", 0, -1), "obs_point = n_xyz": _set("point", 3, 20),
           "obs_point = n_idp": _set("point", 159, 20), "obs_point = -1": _set("point", 100, -1), "obs_kind = 2": _set("kind", 50, 2), "obs_kind = -1": _set("kind", 50, -1),
           "idp_host = n_frames": _set("host", 7, 6), "idp_host = -1": _set("host", 19, -1), "rho = 0": _set("rho", 4, 0.0), "rho < 0": _set("rho", 4, -0.1),
           "rho NaN": _set("rho", 4, np.nan), "scale = 0": _set("S", (3, 7), 0.0), "scale NaN": _set("S", (5, 7), np.nan), "fx = 0": _set("cam", 0, 0.0),
           "fy = 0": _set("cam", 1, 0.0), "free-mask bit 9": _count("cam_free", 1 << 9), "n_frames < 0": _count("frames", -1), "n_frames = 0": _count("frames", 0),
           "n_xyz < 0": _count("xyz", -1), "n_idp < 0": _count("idp", -1), "n_obs < 0": _count("obs", -1)}
    bad.update(("%s NULL" % key, _null(key)) for key in ("S", "dof", "xyz", "host", "anchor", "rho", "kind", "point", "frame", "xy"))
    for what, mutate in bad.items():
        st, clean, launched = _raw_solve(ctx, mutate)
        assert st == 1, (what, st)  # GH_ERR_ARG
        assert clean and not launched, (what, clean, launched)
    st, clean, launched = _raw_solve(ctx, lambda a, n, null: None, sphere=True)   # intrinsics with the sphere projection
    assert st == 1 and clean and not launched
    # the same call is taken once the arrays hold the base graph, and the context is usable afterwards
    def restore(a, n, null):
        a["S"][:], a["xyz"][:], a["rho"][:] = gc.CASES["base"]["start"], gc.CASES["base"]["problem"]["xyz"][0], gc.CASES["base"]["problem"]["idp"][2]
    st, clean, launched = _raw_solve(ctx, restore, with_cam=False)
    assert st == 0 and not clean and "gr_obs_lin" in launched
    compare(gpu_solve(ctx, gc.CASES["base"]), oracle_runs["base"], "base")
