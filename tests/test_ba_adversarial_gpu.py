"""gh_ba_solve, gh_ba_graph_* and gh_ba_pnp (gslam_amd/csrc/ba.hip) on the census of tests/ba_adversarial_cases.py, against
oracle/ba_oracle.c.  The oracle itself is pinned to independent references in tests/test_ba_adversarial_oracle.py.

Bars (those of tests/test_ba_gpu.py and tests/ba_parity.py): identical status / iterations / accepted / termination /
trace length, the same accept / reject at every iteration, radius 1e-9 relative, `inf` candidate costs in the same places,
costs to 1e-9 cost + 1e-18 (one_camera_fixed and two_cams_one_point end near 1e-24), state to max(1e-8, 8 x the case's
yardstick) -- ba_adversarial_cases.YARDSTICK, how far FMA contraction alone moves the oracle: 1e-8 everywhere except
gauge_free (2.9e-5: the null space of the free gauge carries the rounding), which is held to the gauge-invariant statement
as well: the oracle's cost at the GPU's state is the GPU's final cost to 1e-12.  Fixed cameras, fixed points, the
translation of a camera whose translation is masked, and points nothing observes come back bit for bit; whatever was
finite going in is finite coming out.

Non-finite cases.  No device-side wait of a solve depends on a value a NaN can reach (read off the code, not probed):
  - ba_enqueue_step launches the same kernels whatever the data holds; the bad-damping flag (`!(det > 0)`) and the pivot
    flag (`!(d > 0)`) are written and read on the host only after the iteration's one synchronisation;
  - ba_wait_verdict polls a stamp that reduce_publish_kernel writes unconditionally, and is bounded;
  - the single-launch factorisation (chol.hip) waits on arrival counters that every publishing wave increments after its
    stores, bad pivot or not (panel16_factor only sets a flag and goes on), each wait bounded with a common abort word;
  - the single-launch back-substitution hands over the values themselves against a sentinel (0xFFF8BEEFFFF8BEEF): a
    computed value with that bit pattern is published as the canonical NaN instead, so a NaN solution cannot be taken
    for "not there yet", and that wait is bounded too;
  - the gradient maximum goes through fmax / `> 0`, which drop a NaN on both sides (the oracle's fmax does the same).
So the four cases run here, once each."""
import ctypes as C

import numpy as np
import pytest

import ba_adversarial_cases as bc
import oracle_lib

pytestmark = pytest.mark.gpu

COST_RTOL, COST_ATOL, RADIUS_RTOL = 1e-9, 1e-18, 1e-9


def state_bar(name):
    return max(1e-8, 8 * bc.YARDSTICK.get(name, 0.0))


def _oracle_opts(case):
    return oracle_lib.ba_options(huber=case["huber"], max_iterations=case["max_iterations"])


def _gpu_opts(case, deterministic=1):
    from gslam_amd import ba
    return ba.default_options(huber_delta=case["huber"], max_iterations=case["max_iterations"], deterministic=deterministic)


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """The oracle's solve of every case, once."""
    return dict((name, oracle.ba_solve(bc.CASES[name]["graph"], _oracle_opts(bc.CASES[name]), threads=4)) for name in bc.NAMES)


def _solve(ctx, name, deterministic=1):
    from gslam_amd import ba
    case = bc.CASES[name]
    got = ba.solve(ctx, case["graph"], _gpu_opts(case, deterministic))
    solver, tiles, span = ctx.last_ba_solver()
    border, reordered = ctx.last_ba_order()
    print("%s (deterministic=%d): route %s, %d tiles, camera span %d, %d border cameras, reordered %d, %d border points; %d iterations" % (
        name, deterministic, solver, tiles, span, border, reordered, ctx.last_ba_border_points(), got[2].iterations))
    return got


def _close(a, b, rtol, atol=0.0):
    return abs(a - b) <= rtol * abs(b) + atol


def _same_trace(sg, so, name):
    assert (sg.iterations, sg.accepted, sg.termination, sg.trace_len) == (so.iterations, so.accepted, so.termination, so.trace_len), name
    for i in range(so.trace_len):
        assert sg.trace_accepted[i] == so.trace_accepted[i], (name, "accept / reject differs at iteration %d" % i)
        assert _close(sg.trace_radius[i], so.trace_radius[i], RADIUS_RTOL), (name, i)
        if not np.isfinite(so.trace_cost[i]):
            assert sg.trace_cost[i] == so.trace_cost[i] or (np.isnan(sg.trace_cost[i]) and np.isnan(so.trace_cost[i])), (name, i)
        else:
            assert _close(sg.trace_cost[i], so.trace_cost[i], COST_RTOL, COST_ATOL), (name, "cost at iteration %d" % i, sg.trace_cost[i], so.trace_cost[i])


def _untouched(got, g, name):
    poses, pts = got[0], got[1]
    for c in bc.fixed_cams(g):
        assert poses[c].tobytes() == g["cam_pose"][c].tobytes(), (name, "fixed camera", c)
    for c in np.flatnonzero((np.asarray(g["cam_dof"]) & 7) == 0):
        assert poses[c, 4:].tobytes() == g["cam_pose"][c, 4:].tobytes(), (name, "masked translation", c)
    for p in bc.fixed_points(g) + bc.unobserved_points(g):
        assert pts[p].tobytes() == g["point_xyz"][p].tobytes(), (name, "fixed or unobserved point", p)
    assert np.isfinite(poses[np.isfinite(g["cam_pose"])]).all() and np.isfinite(pts[np.isfinite(g["point_xyz"])]).all(), name


def _compare(got, ref, name, oracle=None):
    case = bc.CASES[name]
    g = case["graph"]
    sg, so = got[2], ref[2]
    assert got[3] == ref[3] == 0, name
    assert _close(sg.initial_cost, so.initial_cost, COST_RTOL, COST_ATOL), name
    _same_trace(sg, so, name)
    assert _close(sg.final_cost, so.final_cost, COST_RTOL, COST_ATOL), name
    d = max([float(np.abs(got[k] - ref[k]).max()) for k in (0, 1) if got[k].size])
    print("%s: state differs by %.2e (bar %.2e)" % (name, d, state_bar(name)))
    assert d <= state_bar(name), (name, d)
    _untouched(got, g, name)
    if name in bc.NOTHING_TO_DO or name == "zero_iterations":
        assert got[0].tobytes() == np.ascontiguousarray(g["cam_pose"], np.float64).tobytes() and got[1].tobytes() == np.ascontiguousarray(g["point_xyz"], np.float64).tobytes()
        assert sg.trace_len == 0 and sg.termination == (0 if name == "zero_iterations" else 2) and sg.final_cost == sg.initial_cost
    if name == "gauge_free":
        assert abs(oracle.ba_cost(g, got[0], got[1], huber=case["huber"]) - sg.final_cost) <= 1e-12 * sg.final_cost


def _same_bits(a, b):
    sa, sb = a[2], b[2]
    return (a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            and (sa.iterations, sa.accepted, sa.termination, sa.trace_len) == (sb.iterations, sb.accepted, sb.termination, sb.trace_len)
            and sa.initial_cost == sb.initial_cost and sa.final_cost == sb.final_cost
            and list(sa.trace_cost[:sa.trace_len]) == list(sb.trace_cost[:sb.trace_len])
            and list(sa.trace_radius[:sa.trace_len]) == list(sb.trace_radius[:sb.trace_len])
            and list(sa.trace_accepted[:sa.trace_len]) == list(sb.trace_accepted[:sb.trace_len]))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", bc.FINITE)
def test_census_against_the_oracle(ctx, oracle, oracle_runs, name):
    _compare(_solve(ctx, name), oracle_runs[name], name, oracle)


@pytest.mark.parametrize("name", bc.BOTH_MODES)
def test_deterministic_twice_and_plain_atomics(ctx, oracle, oracle_runs, name):
    a, b = _solve(ctx, name, 1), _solve(ctx, name, 1)
    assert _same_bits(a, b), name
    _compare(_solve(ctx, name, 0), oracle_runs[name], name, oracle)


# ------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("name", bc.NON_FINITE)
def test_non_finite_input(ctx, oracle_runs, name):
    from gslam_amd import ba, hip
    case = bc.CASES[name]
    g = case["graph"]
    ref = oracle_runs[name]
    poses = np.ascontiguousarray(g["cam_pose"], dtype=np.float64).copy()
    pts = np.ascontiguousarray(g["point_xyz"], dtype=np.float64).copy()
    keep = [np.ascontiguousarray(g[k], dtype=dt) for k, dt in (("cam_dof", np.int32), ("obs_cam", np.int32), ("obs_point", np.int32), ("obs_xy", np.float64))]
    pr = hip.BaProblem(len(poses), len(pts), len(keep[1]), ba._ptr(poses), ba._ptr(keep[0]), ba._ptr(pts), None, ba._ptr(keep[1]), ba._ptr(keep[2]),
                       ba._ptr(keep[3]), None)
    sg = hip.BaSummary()
    st = hip.lib.gh_ba_solve(ctx.h, C.byref(pr), C.byref(_gpu_opts(case)), C.byref(sg))
    so = ref[2]
    print("%s: status %d, %d iterations, termination %d, initial cost %r" % (name, st, sg.iterations, sg.termination, sg.initial_cost))
    assert st == (4 if ref[3] == 1 else 0)  # GH_ERR_NUMERIC = the oracle's failure
    _same_trace(sg, so, name)
    if name in ("nan_obs", "inf_obs"):
        assert np.isnan(sg.initial_cost) and np.isnan(so.initial_cost) and (sg.iterations, sg.termination) == (15, 3)
        assert all(np.isinf(sg.trace_cost[i]) for i in range(sg.trace_len))
        assert poses.tobytes() == g["cam_pose"].tobytes() and pts.tobytes() == g["point_xyz"].tobytes()
    else:
        assert _close(sg.initial_cost, so.initial_cost, COST_RTOL) and _close(sg.final_cost, so.final_cost, COST_RTOL)
        for mine, theirs in ((poses, ref[0]), (pts, ref[1])):
            ok = np.isfinite(theirs)
            assert np.isfinite(mine[ok]).all() and np.abs(mine[ok] - theirs[ok]).max() <= 1e-8, name
        _untouched((poses, pts), g, name)
    # the context is as good as before
    _compare(_solve(ctx, "two_cams_one_point"), oracle_runs["two_cams_one_point"], "two_cams_one_point")


# ------------------------------------------------------------------------------------------------ resident graph
def _variant(g, **kw):
    out = dict(g)
    out.update(kw)
    return out


def _graph_run(G, opts):
    s, st = G.solve(opts)
    poses, pts = G.read()
    return poses, pts, s, st


@pytest.mark.parametrize("name", ["unobserved", "dense3_1025"])
def test_resident_graph_updates_one_array_at_a_time(ctx, name):
    from gslam_amd import ba, hip
    case = bc.CASES[name]
    g = dict(case["graph"])
    g.setdefault("point_free", np.ones(len(g["point_xyz"]), np.uint8))
    opts = _gpu_opts(case)
    G = ba.Graph(ctx, g, opts)
    try:
        assert _same_bits(_graph_run(G, opts), ba.solve(ctx, g, opts)), "as created"
        rng = np.random.default_rng(5)
        dof0 = np.zeros(len(g["cam_dof"]), np.int32)
        pfree = g["point_free"].copy()
        pfree[::3] = 0
        oxy = g["obs_xy"] + rng.normal(size=g["obs_xy"].shape) * 1e-3
        # every step: back to the start values (poses and points move in a solve), then ONE more array
        steps = [("cam_dof all zero", dict(cam_dof=dof0), _variant(g, cam_dof=dof0)),
                 ("cam_dof back", dict(cam_dof=g["cam_dof"]), g),
                 ("point_free", dict(point_free=pfree), _variant(g, point_free=pfree)),
                 ("obs_xy", dict(obs_xy=oxy), _variant(g, point_free=pfree, obs_xy=oxy))]
        for what, upd, values in steps:
            G.update(cam_pose=g["cam_pose"])
            G.update(point_xyz=g["point_xyz"])
            G.update(**upd)
            got, want = _graph_run(G, opts), ba.solve(ctx, values, opts)
            assert _same_bits(got, want), (name, what)
            if what == "cam_dof all zero":
                assert got[0].tobytes() == g["cam_pose"].tobytes() and got[2].accepted >= 1
        # refusals: the argument error, and the resident state as it was
        before = G.read()
        info = np.tile(np.eye(2).reshape(-1), (len(g["obs_cam"]), 1))
        assert hip.lib.gh_ba_graph_update(G.g, None, None, None, ba._ptr(info), None, None) == 1
        other = _gpu_opts(case, deterministic=0)
        sm = hip.BaSummary()
        assert hip.lib.gh_ba_graph_solve(G.g, C.byref(other), C.byref(sm)) == 1
        after = G.read()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        G.update(cam_pose=g["cam_pose"])
        G.update(point_xyz=g["point_xyz"])
        assert _same_bits(_graph_run(G, opts), ba.solve(ctx, steps[-1][2], opts)), "after the refusals"
    finally:
        G.close()
    # a graph created WITHOUT point_free refuses one
    bare = dict((k, v) for k, v in g.items() if k != "point_free")
    G = ba.Graph(ctx, bare, opts)
    try:
        first = _graph_run(G, opts)
        ones = np.ones(len(g["point_xyz"]), np.uint8)
        assert hip.lib.gh_ba_graph_update(G.g, None, None, None, None, None, ba._ptr(ones)) == 1
        G.update(cam_pose=g["cam_pose"])
        G.update(point_xyz=g["point_xyz"])
        assert _same_bits(_graph_run(G, opts), first) and _same_bits(first, ba.solve(ctx, bare, opts))
    finally:
        G.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_problems_are_refused_and_left_untouched(ctx, oracle_runs):
    from gslam_amd import ba, hip
    g = bc.CASES["unobserved"]["graph"]
    nc, npnt, no = len(g["cam_dof"]), len(g["point_xyz"]), len(g["obs_cam"])
    dof = np.ascontiguousarray(g["cam_dof"], np.int32)
    pfree = np.ascontiguousarray(g["point_free"], np.uint8)
    oxy = np.ascontiguousarray(g["obs_xy"], np.float64)

    def run(n_cams=nc, n_points=npnt, n_obs=no, null=(), ocam=None, opt=None):
        poses, pts = np.full((nc, 7), 7.25), np.full((npnt, 3), -3.5)  # dirty outputs: they must stay dirty
        oc = np.ascontiguousarray(g["obs_cam"] if ocam is None else ocam, np.int32)
        op = np.ascontiguousarray(g["obs_point"] if opt is None else opt, np.int32)
        a = {"cam_pose": ba._ptr(poses), "cam_dof": ba._ptr(dof), "point_xyz": ba._ptr(pts), "point_free": ba._ptr(pfree), "obs_cam": ba._ptr(oc),
             "obs_point": ba._ptr(op), "obs_xy": ba._ptr(oxy)}
        for k in null:
            a[k] = None
        pr = hip.BaProblem(n_cams, n_points, n_obs, a["cam_pose"], a["cam_dof"], a["point_xyz"], a["point_free"], a["obs_cam"], a["obs_point"], a["obs_xy"], None)
        sm = hip.BaSummary()
        st = hip.lib.gh_ba_solve(ctx.h, C.byref(pr), C.byref(_gpu_opts(bc.CASES["unobserved"])), C.byref(sm))
        return st, (poses == 7.25).all() and (pts == -3.5).all()

    past, minus = g["obs_cam"].copy(), g["obs_point"].copy()
    past[no // 2] = nc
    minus[no - 1] = -1
    bad = {"n_cams = 0": dict(n_cams=0), "n_cams < 0": dict(n_cams=-1), "n_points < 0": dict(n_points=-1), "n_obs < 0": dict(n_obs=-1),
           "cam_pose NULL": dict(null=("cam_pose",)), "cam_dof NULL": dict(null=("cam_dof",)), "obs_cam = n_cams": dict(ocam=past),
           "obs_point = -1": dict(opt=minus), "n_points = 0 with observations": dict(n_points=0)}
    for what, kw in bad.items():
        st, dirty = run(**kw)
        assert st == 1, (what, st)  # GH_ERR_ARG
        assert dirty, what
    _compare(_solve(ctx, "unobserved"), oracle_runs["unobserved"], "unobserved")


# ------------------------------------------------------------------------------------------------ pose-only LM
@pytest.mark.parametrize("name", list(bc.PNP_CASES))
def test_pnp_edges_against_the_oracle(ctx, oracle, name):
    from gslam_amd import ba
    X, m, pose, dof = bc.PNP_CASES[name]
    po, so, _, rc = oracle.ba_pnp(X, m, pose, dof=dof, opts=oracle_lib.ba_options(max_iterations=20))
    pg, sg, _ = ba.pnp(ctx, X, m, pose, dof=dof, options=ba.default_options(max_iterations=20))
    assert rc == 0 and _close(sg.initial_cost, so.initial_cost, COST_RTOL, COST_ATOL) and _close(sg.final_cost, so.final_cost, COST_RTOL, COST_ATOL)
    _same_trace(sg, so, name)
    assert np.abs(pg - po).max() <= 1e-8
    if name in bc.PNP_NOTHING_TO_DO:
        assert pg.tobytes() == np.asarray(pose, np.float64).tobytes() and (sg.iterations, sg.termination, sg.trace_len) == (0, 2, 0)
    if dof == 7:
        assert pg[4:].tobytes() != pose[4:].tobytes() and np.abs(pg[:4] - pose[:4]).max() <= 4e-16
