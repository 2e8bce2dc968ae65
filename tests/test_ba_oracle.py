"""CPU checks of the BA oracle: pose algebra pinned to the reference's own SE3 (golden vectors
generated through oracle/_ref from /root/reference/GSLAM/core/SE3.h), dense Cholesky vs numpy, and
LM behaviour on small synthetic graphs."""
import os

import numpy as np
import pytest

import oracle_lib
from gslam_amd.ba_synth import make_graph, quat_to_R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "se3_reference.npz")


def _ref_to_ours(p):  # reference stream order tx ty tz qx qy qz qw -> qx qy qz qw tx ty tz
    return np.concatenate([p[3:], p[:3]])


def test_se3_exp_matches_reference_golden(oracle):
    g = np.load(GOLD)
    for xi, pose in zip(g["xi"], g["poses"]):
        # the reference evaluates (1-cos t)/t^2 unguarded and loses digits for tiny t (SE3.h:284-285):
        # samples 0/1 (t ~ 1e-6 / 1e-3) are only comparable to ~1e-9
        atol = 1e-12 if np.linalg.norm(xi[3:]) > 1e-2 else 2e-9
        assert np.allclose(oracle.se3_exp(xi), _ref_to_ours(pose), rtol=0, atol=atol)


def test_se3_retract_matches_reference_mul(oracle):
    """T * exp(xi) against the reference's operator* (SE3.h:120-123) applied to its own exp."""
    g = np.load(GOLD)
    for i in range(63):
        a = _ref_to_ours(g["poses"][i])
        got = oracle.se3_retract(a, g["xi"][i + 1])
        exp = _ref_to_ours(g["muls"][i])  # poses[i] * poses[i+1], poses[i+1] == exp(xi[i+1])
        atol = 1e-12 if np.linalg.norm(g["xi"][i + 1][3:]) > 1e-2 else 2e-9
        assert np.allclose(got, exp, rtol=0, atol=atol)


def test_se3_exp_zero_rotation_is_finite(oracle):
    """The reference's SE3::exp returns NaN for w == 0; the oracle is guarded."""
    p = oracle.se3_exp(np.array([1.0, 2.0, 3.0, 0, 0, 0]))
    assert np.array_equal(p, np.array([0, 0, 0, 1, 1, 2, 3.0]))
    p = oracle.se3_exp(np.array([1.0, 2.0, 3.0, 1e-9, 0, 0]))
    assert np.all(np.isfinite(p)) and abs(p[4] - 1) < 1e-8


def test_world_to_cam_matches_reference_inverse_apply(oracle):
    """cost at the reference-transformed measurement must be zero: m = (T^-1 X).xy / z."""
    g = np.load(GOLD)
    for i in range(16):
        pose = _ref_to_ours(g["poses"][i])
        inv = g["invs"][i]
        R = quat_to_R(inv[None, 3:])[0]
        X = g["pts"][i] + np.array([0, 0, 20.0])
        Xc = R @ X + inv[:3]
        if Xc[2] < 0.1:
            continue
        graph = {"cam_pose": pose[None], "point_xyz": X[None], "obs_cam": np.array([0], np.int32),
                 "obs_point": np.array([0], np.int32), "obs_xy": (Xc[:2] / Xc[2])[None]}
        assert oracle.ba_cost(graph) < 1e-24


def test_potrf_against_numpy(oracle):
    rng = np.random.default_rng(0)
    for n in (1, 5, 64, 130, 300):
        M = rng.standard_normal((n, n))
        A = M @ M.T + n * np.eye(n)
        b = rng.standard_normal(n)
        L, x, info = oracle.potrf_solve(A, b, threads=2)
        assert info == 0
        assert np.allclose(L, np.linalg.cholesky(A), atol=1e-10)
        assert np.allclose(A @ x, b, atol=1e-9)
    _, _, info = oracle.potrf_solve(-np.eye(3), np.ones(3))
    assert info == 1


def test_lm_converges_to_ground_truth_without_noise(oracle):
    g = make_graph(8, 120, n_obs_per_point=4, seed=3, noise=0.0, outlier_frac=0.0)
    poses, pts, s, rc = oracle.ba_solve(g, oracle_lib.ba_options(huber=0.01, max_iterations=60))
    assert rc == 0 and s.final_cost < 1e-16 * max(1.0, s.initial_cost) + 1e-18
    assert s.accepted >= 3 and s.iterations <= 60


def test_lm_noisy_with_outliers(oracle):
    g = make_graph(12, 300, n_obs_per_point=5, seed=1)
    c0 = oracle.ba_cost(g)
    poses, pts, s, rc = oracle.ba_solve(g, oracle_lib.ba_options(max_iterations=50))
    assert rc == 0 and abs(s.initial_cost - c0) < 1e-12 * c0
    # outliers keep the robust cost well above zero: the bar is the cost at the ground truth
    assert s.final_cost < oracle.ba_cost(g, g["cam_pose_gt"], g["point_xyz_gt"]) < 0.5 * s.initial_cost
    assert s.termination in (1, 2)
    assert np.array_equal(poses[0], g["cam_pose"][0])  # fixed camera untouched
    tr = [s.trace_cost[i] for i in range(s.trace_len)]
    acc = [s.trace_accepted[i] for i in range(s.trace_len)]
    accepted_costs = [c for c, a in zip(tr, acc) if a]
    assert all(b < a for a, b in zip([s.initial_cost] + accepted_costs[:-1], accepted_costs))
    # cost at the returned state equals the reported final cost
    assert abs(oracle.ba_cost(g, poses, pts) - s.final_cost) <= 1e-12 * s.final_cost


def test_dof_mask_and_fixed_points(oracle):
    g = make_graph(6, 80, n_obs_per_point=4, seed=5)
    g["cam_dof"] = np.array([0, 7, 63, 63, 56, 63], np.int32)  # fixed, translation-only, ..., rotation-only
    g["point_free"] = np.ones(80, np.uint8)
    g["point_free"][:10] = 0
    poses, pts, s, rc = oracle.ba_solve(g, oracle_lib.ba_options(max_iterations=30))
    assert rc == 0 and s.final_cost < s.initial_cost
    assert np.array_equal(poses[0], g["cam_pose"][0])
    assert np.allclose(poses[1, :4], g["cam_pose"][1, :4], atol=1e-15)  # rotation frozen
    assert np.allclose(poses[4, 4:], g["cam_pose"][4, 4:], atol=1e-15)  # translation frozen
    assert np.array_equal(pts[:10], g["point_xyz"][:10])
    assert not np.array_equal(pts[10:], g["point_xyz"][10:])


def test_information_matrix_scales_cost(oracle):
    g = make_graph(5, 40, n_obs_per_point=3, seed=7)
    c1 = oracle.ba_cost(g, huber=0.0)
    g["obs_info"] = np.tile(np.array([4.0, 0, 0, 4.0]), (len(g["obs_cam"]), 1))
    assert abs(oracle.ba_cost(g, huber=0.0) - 4 * c1) < 1e-12 * c1


def behind_camera_graph():
    """One fixed camera at the origin, one free point 1 cm in front of it whose Gauss-Newton step lands BEHIND the
    camera: dropping the observation there would make the cost 0 and LM would accept a point behind the camera."""
    return {"cam_pose": np.array([[0, 0, 0, 1.0, 0, 0, 0]]), "cam_dof": np.array([0], np.int32),
            "point_xyz": np.array([[0.01, 0, 0.01]]), "obs_cam": np.array([0], np.int32),
            "obs_point": np.array([0], np.int32), "obs_xy": np.array([[5.0, 0.0]])}


def test_step_that_moves_a_point_behind_its_camera_is_rejected(oracle):
    g = behind_camera_graph()
    poses, pts, s, rc = oracle.ba_solve(g, oracle_lib.ba_options(huber=0.0, max_iterations=30))
    assert rc == 0 and s.trace_accepted[0] == 0 and np.isinf(s.trace_cost[0])
    assert pts[0, 2] > 1e-9 and s.final_cost < 1e-20 * s.initial_cost
    assert abs(pts[0, 0] / pts[0, 2] - 5.0) < 1e-9


def test_full_c4_state_sensitivity_to_rounding(oracle):
    """How far rounding alone moves the C4 solution: the oracle compiled with FMA contraction (oracle/liboracle_fma.so, same
    source) against itself.  Costs agree to 1e-12 at every iteration, the accept/reject sequence is identical and the final
    states agree to ~1e-11 (measured 1.6e-12 .. 1.2e-11 in pose over seeds 1-3) -- which is why the GPU-vs-oracle state bar
    at full C4 is the 1e-8 of the small graphs (tests/test_full_configs_gpu.py::STATE_ATOL_FULL).  On the generator of
    rounds 1-3 (303 of 500 cameras unobserved) the same experiment gave 1.1e-6."""
    import os
    fma = oracle_lib.Oracle(os.path.join(oracle_lib.ROOT, "oracle", "liboracle_fma.so"))
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1)
    a = oracle.ba_solve(g, oracle_lib.ba_options(max_iterations=40), threads=8)
    b = fma.ba_solve(g, oracle_lib.ba_options(max_iterations=40), threads=8)
    sa, sb = a[2], b[2]
    assert (sa.iterations, sa.accepted, sa.termination) == (sb.iterations, sb.accepted, sb.termination)
    for i in range(sa.trace_len):
        assert sa.trace_accepted[i] == sb.trace_accepted[i]
        assert abs(sa.trace_cost[i] - sb.trace_cost[i]) <= 1e-12 * sa.trace_cost[i]
    d_pose, d_pts = np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()
    assert d_pose <= 1e-9 and d_pts <= 1e-9


def test_bench_graphs_are_well_posed():
    """every camera of the C4 graph sees points, evenly, and the reduced camera system is a band."""
    from gslam_amd.ba_synth import graph_census
    c = graph_census(make_graph(500, 50000, n_obs_per_point=6, seed=1))
    assert c["cams_observed"] == 500 and c["obs_per_cam_min"] >= 50
    assert c["obs_per_cam_max"] <= 4 * c["obs_per_cam_median"]
    assert 0.05 < c["s_block_fill"] < 0.15


def test_full_c4_oracle_camera_order_sensitivity(oracle):
    """How far the camera ORDER alone moves the oracle's C4 solution: the same graph with the cameras shuffled (and the shuffle
    undone afterwards).  The GPU-vs-oracle comparisons on shuffled graphs (tests/test_ba_solver_paths_gpu.py) hold the GPU to
    cost 1e-9 / state 1e-8 of the oracle on the shuffled graph; this shows the oracle itself moves far less than that (measured:
    23 of 23 iterations accepted both ways, costs within 3.5e-13, poses within 8e-13, points within 7.0e-11)."""
    from test_ba_order import _shuffle
    threads = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1)
    h, new_of_old = _shuffle(g, 1)
    a = oracle.ba_solve(g, oracle_lib.ba_options(max_iterations=40), threads=threads)
    b = oracle.ba_solve(h, oracle_lib.ba_options(max_iterations=40), threads=threads)
    sa, sb = a[2], b[2]
    assert a[3] == 0 and b[3] == 0
    assert (sa.iterations, sa.accepted, sa.termination, sa.trace_len) == (sb.iterations, sb.accepted, sb.termination, sb.trace_len)
    for i in range(sa.trace_len):
        assert sa.trace_accepted[i] == sb.trace_accepted[i]
        assert abs(sa.trace_cost[i] - sb.trace_cost[i]) <= 1e-12 * sa.trace_cost[i]
    assert abs(sa.initial_cost - sb.initial_cost) <= 1e-12 * sa.initial_cost
    assert abs(sa.final_cost - sb.final_cost) <= 1e-12 * sa.final_cost
    d_pose, d_pts = np.abs(b[0][new_of_old] - a[0]).max(), np.abs(b[1] - a[1]).max()
    print("oracle, shuffled vs in order: %d iterations, %d accepted, pose %.2g, points %.2g" % (sa.iterations, sa.accepted, d_pose,
                                                                                            d_pts))
    assert d_pose <= 1e-9 and d_pts <= 1e-9
