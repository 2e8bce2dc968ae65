"""gh_pg_solve and gh_graph_solve (posegraph.hip, bsparse.hip) on the census of tests/pg_adversarial_cases.py: every
graph through every route against oracle/pg_oracle.c, and the invariants of the problem GPU against GPU.  The oracle
itself is pinned to independent references in tests/test_pg_adversarial_oracle.py.

Bars: those of tests/pg_parity.py (initial cost 1e-12, identical iteration count / termination / accept-reject
sequence, radius and cost 1e-9, frames 1e-7, fixed frames bit-identical), unchanged.  Bitwise where it says so.

Routes: the dense system (GSLAM_HIP_PG_SPARSE_MIN=1000000); the block-sparse solver forced on (GSLAM_HIP_PG_SPARSE_MIN=0)
with a dense root of at least GSLAM_HIP_PG_ROOT = 1 and 4 keyframes -- the profile must show bs_factor_cols wherever the
symbolic factorisation (gslam_amd.posegraph.bs_symbolic, host only) eliminates a column at all; gh_graph_solve with no
landmarks.  Every route twice, the two runs bit-identical.

MAX_IT.  Every case runs 40 iterations but four, which run one (linearise, assemble, solve, trial step, decision -- every
kernel -- and all bars hold on it):
    branch_grid_t1, branch_grid_t1e4, scales, info_aniso.
From the second linearisation on these four cannot hold the bars, and not through a fault of the kernels: the
Jacobians are central differences with h = 1e-6 (the specification), which multiply the last-bit differences between
device and glibc sin / cos / exp by 1 / 2h = 5e5 times the size of the terms that cancel in the residual.
  - branch grid: the closed form of sim3_abc just above theta = 1e-5 carries 1.7e-12 |t| of cancellation noise
    ((1 - cos theta) / theta^2; 2.2e-13 |t| at theta = 1e-4, tests/test_pg_adversarial_oracle.py), which is 1e-6 |t| in a
    Jacobian entry.  The graph converges to zero residual, so its residual rotations pass through that band.
  - scales: (t_j - t_i) / s_i is 1e7 in size and cancels to 32: 1e7 * 1e-16 / 2e-6 = 5e-4 in a Jacobian entry.
  - info_aniso: informations of condition 1e8 (eigenvalues 1e-4 .. 1e4) turn a frame difference d into a cost
    difference of sqrt(2 cost * 1e4) d until the gradient has vanished; d = 5e-10, far inside the 1e-7 bar on the frames,
    exceeds the 1e-9 bar on the cost.
Measured on the dense route, relative difference of the per-iteration cost, GPU against oracle (frames after the run):
    iteration         0        1        2        3        last (40 iterations)   frames after 1 / 40 iterations
    branch_grid_t1    4.8e-13  2.4e-09  1.2e-08  3.7e-08  3.7e-08 (cost 5e-17)   8.2e-11 / 6.2e-11
    branch_grid_t1e4  1.2e-12  2.1e-06  4.0e-07  4.5e-06  1.6e-06                8.6e-08 / 1.0e-02  (translations of 1e4)
    scales            1.4e-11  2.7e-04  3.8e-04  9.4e-04  2.4e-03                5.4e-09 / 2.3e-02  (translations of 1e4)
    info_aniso        5.0e-11  1.5e-09  1.8e-09  3.1e-11  6.5e-14                3.5e-12 / 1.4e-09
The iteration counts, terminations and accept / reject sequences of all four were identical over the 40 iterations.  The
initial cost holds its 1e-12 bar everywhere, theta = 1.01e-5 included (on the 80 single-edge graphs GPU and oracle agree bit for bit),
so the bar of its own that this class might have needed is not used.

near_pi: the frames on the edges with residual rotations of 3.0 and 3.1405 rad have no rotational degree of freedom.
With free rotations the solve walks those residuals towards and across the cut of the logarithm at pi (three rejected
steps, 26 iterations), and the radius left its 1e-9 bar at iteration 5 (1.4e-9) after a cost difference of 6.1e-10.

branch_grid_t1e4 keeps the translations and scales of its frames fixed (dof = rotation): one step moves a free frame by
1e4, and the dense and the block-sparse solve then agree with the oracle to 8.6e-8 and 1.7e-7 on those translations --
1e-11 relative, the rounding of a 287 x 287 solve -- against an absolute bar of 1e-7.

The per-edge solves of the branch grid (80 two-frame graphs) compare the initial cost (see the test)."""
import numpy as np
import pytest

import oracle_lib
import pg_adversarial_cases as pc
from pg_parity import compare_runs

pytestmark = pytest.mark.gpu

ROUTES = ("dense", "sparse_root1", "sparse_root4", "graph_solve")
MAX_IT = {"branch_grid_t1": 1, "branch_grid_t1e4": 1, "scales": 1, "info_aniso": 1}


def _set_route(monkeypatch, route):
    if route.startswith("sparse"):
        monkeypatch.setenv("GSLAM_HIP_PG_SPARSE_MIN", "0")
        monkeypatch.setenv("GSLAM_HIP_PG_ROOT", route[len("sparse_root"):])
    else:
        monkeypatch.setenv("GSLAM_HIP_PG_SPARSE_MIN", "1000000")


def _solver(route):
    from gslam_amd import posegraph
    if route != "graph_solve":
        return posegraph.solve

    def solve(ctx, start, dof, prob, options):
        S, xyz, rho, sm, st = posegraph.solve_graph(ctx, start, dof, prob, options)
        return S, sm, st
    return solve


def _pairs(problem):
    seen = sorted(set((max(i, j), min(i, j)) for _, i, j, _ in pc.all_edges(problem) if j >= 0))
    return np.array([p[0] for p in seen], np.int32), np.array([p[1] for p in seen], np.int32)


def _profiled(ctx, fn):
    ctx.prof_enable(True)
    try:
        out = fn()
        names = set(ctx.prof_collect().keys())
    finally:
        ctx.prof_enable(False)
    return out, names


def _same_bits(a, b):
    (Sa, sa, sta), (Sb, sb, stb) = a, b
    return (sta == stb and Sa.tobytes() == Sb.tobytes() and (sa.iterations, sa.accepted, sa.termination) == (sb.iterations, sb.accepted, sb.termination)
            and sa.initial_cost == sb.initial_cost and sa.final_cost == sb.final_cost
            and list(sa.trace_cost[:sa.trace_len]) == list(sb.trace_cost[:sb.trace_len])
            and list(sa.trace_radius[:sa.trace_len]) == list(sb.trace_radius[:sb.trace_len]))


def _run(ctx, graph, name, route="dense"):
    from gslam_amd import ba
    start, dof, prob = graph
    return _solver(route)(ctx, start, dof, prob, ba.default_options(max_iterations=MAX_IT.get(name, 40)))


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """The oracle's solve of every case, once."""
    return dict((name, oracle.pg_solve(*pc.CASES[name], oracle_lib.ba_options(max_iterations=MAX_IT.get(name, 40)), threads=4))
                for name in pc.NAMES)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", pc.NAMES)
def test_census_against_the_oracle(ctx, oracle_runs, monkeypatch, name, route):
    from gslam_amd import posegraph
    _set_route(monkeypatch, route)
    start, dof, prob = pc.CASES[name]
    got, kernels = _profiled(ctx, lambda: _run(ctx, pc.CASES[name], name, route))
    again = _run(ctx, pc.CASES[name], name, route)
    ref = oracle_runs[name]
    print("%s / %s: initial cost gpu %.17g oracle %.17g; %d iterations; frames differ by %.2e" % (
        name, route, got[1].initial_cost, ref[1].initial_cost, got[1].iterations, np.abs(got[0] - ref[0]).max()))
    compare_runs(got, ref, start, fixed=pc.fixed_frames(dof) + pc.UNTOUCHED.get(name, []))
    assert _same_bits(got, again)
    if route.startswith("sparse"):
        prow, pcol = _pairs(prob)
        sym = posegraph.bs_symbolic(len(start), prow, pcol, root_min=int(route[len("sparse_root"):]))
        assert ("bs_factor_cols" in kernels) == (sym["ns"] > 0) and "pg_damp" not in kernels
    else:
        assert "bs_factor_cols" not in kernels
    if name in pc.NOTHING_TO_DO:
        sm = got[1]
        assert (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (0, 0, 2, 0) and got[0].tobytes() == start.tobytes()
        assert sm.initial_cost == sm.final_cost and abs(sm.final_cost - ref[1].final_cost) <= 1e-12 * ref[1].final_cost


@pytest.mark.parametrize("route", ("dense", "sparse_root1"))
def test_negated_quaternions_are_the_same_problem(ctx, monkeypatch, route):
    _set_route(monkeypatch, route)
    a, b = _run(ctx, pc.CASES["neg_w"], "neg_w", route), _run(ctx, pc.TWINS["neg_w"], "neg_w", route)
    flipped = b[0].copy()
    flipped[:, :4] *= -1.0
    compare_runs(a, (flipped, b[1], b[2]), pc.CASES["neg_w"][0], fixed=[0])
    assert (pc.CASES["neg_w"][0][:, 3] < 0).all() and (pc.TWINS["neg_w"][0][:, 3] > 0).all()


@pytest.mark.parametrize("route", ("dense", "sparse_root1", "graph_solve"))
def test_explicit_identity_informations_equal_none_bitwise(ctx, monkeypatch, route):
    _set_route(monkeypatch, route)
    assert _same_bits(_run(ctx, pc.CASES["info_identity"], "info_identity", route), _run(ctx, pc.TWINS["info_identity"], "info_identity", route))


@pytest.mark.parametrize("route", ("dense", "sparse_root4"))
def test_an_edge_with_zero_information_is_no_edge(ctx, monkeypatch, route):
    _set_route(monkeypatch, route)
    a, b = _run(ctx, pc.CASES["info_zero_edge"], "", route), _run(ctx, pc.TWINS["info_zero_edge"], "", route)
    compare_runs(a, b, pc.CASES["info_zero_edge"][0], fixed=[0])


@pytest.mark.parametrize("route", ("dense", "sparse_root1", "sparse_root4"))
@pytest.mark.parametrize("name", ["both_ways", "hub", "two_components", "dof_masks", "isolated", "info_mixed", "near_pi"])
def test_edge_order_and_frame_labels_do_not_matter(ctx, monkeypatch, name, route):
    """A permutation of the edges inside each list, and a relabelling of the frames (prow / pcol, the flips and the
    block-sparse elimination order all change), against the graph as it stands."""
    _set_route(monkeypatch, route)
    start, dof, prob = pc.CASES[name]
    fixed = pc.fixed_frames(dof) + pc.UNTOUCHED.get(name, [])
    base = _run(ctx, pc.CASES[name], name, route)
    shuffled = _run(ctx, (start, dof, pc.permute_edges(prob, seed=5)), name, route)
    compare_runs(shuffled, base, start, fixed=fixed)
    s2, d2, p2, perm = pc.relabel_frames(start, dof, prob, seed=6)
    S2, sm2, st2 = _run(ctx, (s2, d2, p2), name, route)
    compare_runs((S2[perm], sm2, st2), base, start, fixed=fixed)
    s3, d3, p3, perm3 = pc.relabel_frames(start, dof, pc.permute_edges(prob, seed=7), seed=8)
    S3, sm3, st3 = _run(ctx, (s3, d3, p3), name, route)
    compare_runs((S3[perm3], sm3, st3), base, start, fixed=fixed)


def test_branch_grid_edge_by_edge(ctx, oracle, monkeypatch):
    """The 80 edges of the branch grid as two-frame graphs: one residual each, through every branch of sim3_abc and
    rot_log.  The initial cost is held to the oracle's at 1e-12, with the status, the iteration count and the decision
    on the step.  The cost AFTER the step is not compared: one damped Gauss-Newton step takes a single edge to 1e-8 of
    its cost, where the 1e-6 noise of a finite-difference Jacobian is all that is left of it."""
    from gslam_amd import ba, posegraph
    _set_route(monkeypatch, "dense")
    worst = {}
    for name, ang, sig, (start, dof, prob) in pc.branch_grid_edges():
        So, so, sto = oracle.pg_solve(start, dof, prob, oracle_lib.ba_options(max_iterations=1), threads=1)
        Sg, sg, stg = posegraph.solve(ctx, start, dof, prob, ba.default_options(max_iterations=1))
        rel = abs(sg.initial_cost - so.initial_cost) / so.initial_cost
        worst[ang] = max(worst.get(ang, 0.0), rel)
        assert stg == sto == 0 and rel <= 1e-12, (name, rel)
        assert (sg.iterations, sg.accepted, sg.trace_len, sg.trace_accepted[0]) == (so.iterations, so.accepted, so.trace_len, so.trace_accepted[0]), name
        assert Sg[0].tobytes() == start[0].tobytes() and sg.final_cost < sg.initial_cost, name
    print("worst relative difference of the initial cost per residual angle:", dict((k, "%.1e" % v) for k, v in worst.items()))


def _raw_solve(ctx, start, dof, prob):
    import ctypes as C
    from gslam_amd import ba, hip, posegraph
    S = np.ascontiguousarray(start, dtype=np.float64).copy()
    d = np.ascontiguousarray(dof, dtype=np.int32)
    keep, pr, sm = [S, d], hip.PgProblem(), hip.BaSummary()
    posegraph._fill_pose_part(pr, S, d, prob, keep)
    opts = ba.default_options(max_iterations=5)
    return hip.lib.gh_pg_solve(ctx.h, C.byref(pr), C.byref(opts), C.byref(sm)), S


def test_bad_graphs_are_refused_and_left_untouched(ctx):
    start, dof, prob = pc.CASES["info_identity"]
    bad = []
    for key in ("se3", "sim3"):
        for what in ("self_edge", "negative_index", "index_past_the_end"):
            val = [np.array(a).copy() if a is not None else None for a in prob[key]]
            val[1][3] = {"self_edge": val[0][3], "negative_index": -1, "index_past_the_end": len(start)}[what]
            bad.append((key + "_" + what, start, dict(prob, **{key: tuple(val)})))
            val = [np.array(a).copy() if a is not None else None for a in prob[key]]
            val[0][0] = {"self_edge": val[1][0], "negative_index": -5, "index_past_the_end": len(start) + 7}[what]
            bad.append((key + "_first_" + what, start, dict(prob, **{key: tuple(val)})))
    gps = [np.array(a).copy() if a is not None else None for a in prob["gps"]]
    gps[0][1] = len(start)
    bad.append(("gps_index_past_the_end", start, dict(prob, gps=tuple(gps))))
    for scale in (0.0, -1.0):
        val = [np.array(a).copy() if a is not None else None for a in prob["sim3"]]
        val[2][2, 7] = scale
        bad.append(("sim3_measurement_scale_%g" % scale, start, dict(prob, sim3=tuple(val))))
        s2 = start.copy()
        s2[4, 7] = scale
        bad.append(("frame_scale_%g" % scale, s2, prob))
    for name, s, p in bad:
        st, S = _raw_solve(ctx, s, dof, p)
        assert st == 1, (name, st)  # GH_ERR_ARG
        assert S.tobytes() == np.ascontiguousarray(s, dtype=np.float64).tobytes(), name
    st, S = _raw_solve(ctx, start, dof, prob)
    assert st == 0 and S.tobytes() != start.tobytes()
