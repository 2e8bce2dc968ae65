"""GPU parity of the BA solver (HIP, through the C ABI) vs the CPU oracle.
Tolerances (f64 GPU vs f64 oracle, north-star: 'SE3 poses/landmarks to a stated float tolerance'):
  identical LM iteration counts and accept/reject sequence; per-iteration cost 1e-9 relative;
  final quaternion / translation / landmarks 1e-8 absolute (scene scale ~10)."""
import numpy as np
import pytest

import oracle_lib
from gslam_amd.ba_synth import make_graph

pytestmark = pytest.mark.gpu

COST_RTOL = 1e-9
STATE_ATOL = 1e-8


def _compare(oracle, ctx, g, max_it=40, deterministic=1, huber=0.01):
    from gslam_amd import ba
    eo = oracle.ba_solve(g, oracle_lib.ba_options(huber=huber, max_iterations=max_it), threads=4)
    opts = ba.default_options(huber_delta=huber, max_iterations=max_it, deterministic=deterministic)
    gp = ba.solve(ctx, g, opts)
    so, sg = eo[2], gp[2]
    assert gp[3] == 0 and eo[3] == 0
    assert abs(sg.initial_cost - so.initial_cost) <= COST_RTOL * so.initial_cost
    assert sg.iterations == so.iterations and sg.accepted == so.accepted and sg.termination == so.termination
    assert sg.trace_len == so.trace_len
    for i in range(so.trace_len):
        assert sg.trace_accepted[i] == so.trace_accepted[i], f"accept/reject differs at iteration {i}"
        assert abs(sg.trace_radius[i] - so.trace_radius[i]) <= 1e-9 * so.trace_radius[i]
        if np.isinf(so.trace_cost[i]):  # candidate rejected because it moved an observation behind its camera
            assert np.isinf(sg.trace_cost[i])
            continue
        assert abs(sg.trace_cost[i] - so.trace_cost[i]) <= COST_RTOL * max(so.trace_cost[i], 1e-30) + 1e-18
    assert abs(sg.final_cost - so.final_cost) <= COST_RTOL * so.final_cost + 1e-18
    assert np.abs(gp[0] - eo[0]).max() <= STATE_ATOL
    assert np.abs(gp[1] - eo[1]).max() <= STATE_ATOL
    return eo, gp


@pytest.mark.parametrize("deterministic", [1, 0])
def test_ba_parity_small(ctx, oracle, deterministic):
    g = make_graph(12, 300, n_obs_per_point=5, seed=1)
    _compare(oracle, ctx, g, deterministic=deterministic)


def test_ba_parity_medium_c4_over_10(ctx, oracle):
    """C4 / 10: 50 cameras, 5k points, 30k observations, Huber."""
    g = make_graph(50, 5000, n_obs_per_point=6, seed=2)
    eo, gp = _compare(oracle, ctx, g, max_it=30)
    assert gp[2].final_cost < 0.5 * gp[2].initial_cost


def test_ba_parity_noiseless_converges_to_truth(ctx, oracle):
    g = make_graph(8, 120, n_obs_per_point=4, seed=3, noise=0.0, outlier_frac=0.0)
    from gslam_amd import ba
    poses, pts, s, st = ba.solve(ctx, g, ba.default_options(max_iterations=60))
    assert st == 0 and s.final_cost < 1e-18
    # gauge: only camera 0 is fixed, so compare reprojection, not raw coordinates
    assert oracle.ba_cost(g, poses, pts) < 1e-18


def test_ba_parity_dof_masks_fixed_points_information(ctx, oracle):
    g = make_graph(6, 80, n_obs_per_point=4, seed=5)
    g["cam_dof"] = np.array([0, 62, 63, 7, 56, 63], np.int32)
    g["point_free"] = np.ones(80, np.uint8)
    g["point_free"][:10] = 0
    rng = np.random.default_rng(1)
    a = rng.uniform(0.5, 2.0, len(g["obs_cam"]))
    b = rng.uniform(-0.2, 0.2, len(g["obs_cam"]))
    g["obs_info"] = np.stack([a, b, b, a + 0.5], axis=1)
    eo, gp = _compare(oracle, ctx, g, max_it=30)
    assert np.array_equal(gp[0][0], g["cam_pose"][0])
    assert np.allclose(gp[0][3, :4], g["cam_pose"][3, :4], atol=1e-15)
    assert np.allclose(gp[0][4, 4:], g["cam_pose"][4, 4:], atol=1e-15)
    assert np.array_equal(gp[1][:10], g["point_xyz"][:10])


def test_ba_same_camera_twice_per_point(ctx, oracle):
    """A point observed twice by the same camera (duplicate block) must still match the oracle."""
    g = make_graph(6, 60, n_obs_per_point=3, seed=9)
    extra = 20
    g["obs_cam"] = np.concatenate([g["obs_cam"], g["obs_cam"][:extra]])
    g["obs_point"] = np.concatenate([g["obs_point"], g["obs_point"][:extra]])
    g["obs_xy"] = np.concatenate([g["obs_xy"], g["obs_xy"][:extra] + 1e-3])
    _compare(oracle, ctx, g, max_it=25, deterministic=1)
    _compare(oracle, ctx, g, max_it=25, deterministic=0)


def test_ba_step_behind_the_camera_is_rejected(ctx, oracle):
    from test_ba_oracle import behind_camera_graph
    g = behind_camera_graph()
    eo, gp = _compare(oracle, ctx, g, max_it=30, huber=0.0)
    assert np.isinf(gp[2].trace_cost[0]) and gp[2].trace_accepted[0] == 0
    assert gp[1][0, 2] > 1e-9 and gp[2].final_cost < 1e-20 * gp[2].initial_cost


@pytest.mark.parametrize("n_cams,n_points", [(40, 3000), (130, 4000)])
def test_ba_deterministic_mode_is_bitwise_reproducible(ctx, n_cams, n_points):
    """Two solves on one context.  18 000 observations stay just under the 20 000 at which the team-built index lists, the
    staged early upload (second solve: the arena of the first is there) and the device-built pair lists start; 24 000 take them."""
    from gslam_amd import ba
    g = make_graph(n_cams, n_points, n_obs_per_point=6, seed=4)
    a = ba.solve(ctx, g, ba.default_options(max_iterations=10, deterministic=1))
    b = ba.solve(ctx, g, ba.default_options(max_iterations=10, deterministic=1))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert [a[2].trace_cost[i] for i in range(a[2].trace_len)] == [b[2].trace_cost[i] for i in range(b[2].trace_len)]


@pytest.mark.parametrize("n", [1, 6, 64, 70, 128, 200, 256, 257, 300, 320, 512, 777, 1024, 1500])
def test_potrf_solve_vs_numpy(ctx, n):
    from gslam_amd import ba
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    b = rng.standard_normal(n)
    L, x, info = ba.potrf_solve(ctx, A, b)
    assert info == 0
    Lr = np.linalg.cholesky(A)
    assert np.abs(L - Lr).max() <= 1e-10 * np.abs(Lr).max()
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b) * np.linalg.cond(A)


@pytest.mark.parametrize("n", [64, 65, 130, 1000, 3000, 3001, 4097, 8192, 8256, 12300, 16500])
def test_backsubstitution_single_launch_matches_the_stepwise_path(ctx, n, monkeypatch):
    """The single-launch back-substitution (one resident workgroup per 64-column block, x handed from block to block
    through agent-scope stores) against the launch-per-step one on the same factor: same sums in a different order."""
    from gslam_amd import ba
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, 64))
    A = M @ M.T / 64.0 + 2.0 * np.eye(n)
    b = rng.standard_normal(n)
    monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", "1")
    L1, x1, info1 = ba.potrf_solve(ctx, A, b)
    x1b = ba.potrf_solve(ctx, A, b)[1]
    monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", "0")
    L0, x0, info0 = ba.potrf_solve(ctx, A, b)
    assert info0 == 0 and info1 == 0 and L0.tobytes() == L1.tobytes()
    assert x1.tobytes() == x1b.tobytes()  # fixed summation order: reproducible run to run
    assert np.abs(x1 - x0).max() <= 1e-13 * np.abs(x0).max()
    assert np.linalg.norm(A @ x1 - b) <= 1e-12 * np.linalg.norm(b)


@pytest.mark.parametrize("n", [16, 64, 80, 128, 192, 256, 320, 1024, 2000, 3008, 3200])
def test_single_launch_factorisation_matches_the_launch_per_step_path(ctx, n, monkeypatch):
    """potrf_flow_kernel (one launch of resident workgroups handing tiles to each other, left-looking accumulation in
    MFMA registers) against the launch-per-step factorisation: same factor to rounding, reproducible bit for bit."""
    from gslam_amd import ba
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, 96))
    A = M @ M.T / 96.0 + 2.0 * np.eye(n)
    b = rng.standard_normal(n)
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "1")
    L1, x1, info1 = ba.potrf_solve(ctx, A, b)
    L1b = ba.potrf_solve(ctx, A, b)[0]
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "0")
    L0, x0, info0 = ba.potrf_solve(ctx, A, b)
    assert info0 == 0 and info1 == 0
    assert L1.tobytes() == L1b.tobytes()
    assert np.abs(L1 - L0).max() <= 1e-13 * np.abs(L0).max()
    assert np.abs(L1 - np.linalg.cholesky(A)).max() <= 1e-12 * np.abs(L0).max()
    assert np.linalg.norm(A @ x1 - b) <= 1e-12 * np.linalg.norm(b)


@pytest.mark.parametrize("n", [65, 130, 321])
def test_potrf_solve_with_the_rhs_row_at_sizes_off_the_16_grid(ctx, n, monkeypatch):
    """gh_potrf_solve_dev called directly with lda > n (the right-hand side rides as row n: extra_rows = 1) at n that are no
    multiple of 16, two to six diagonal blocks: every buffer of the solve's workspace then starts where the shared layout
    (dense_solve.h) puts it, on a 128-byte line.  Single-launch kernels on and off, each reproducible bit for bit, right by
    the residual, and the paths agree."""
    import ctypes as C
    import torch
    from gslam_amd import hip
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, 96))
    A = M @ M.T / 96.0 + 2.0 * np.eye(n)
    b = rng.standard_normal(n)
    lda = (n + 1 + 15) // 16 * 16
    cols = np.zeros((n, lda))  # row c = column c of the column-major device matrix; the rows n .. lda - 1 are scratch
    cols[:, :n] = A

    def solve(flow, chain):
        monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", flow)
        monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", chain)
        dA, x, info = torch.from_numpy(cols).cuda(), torch.from_numpy(b).cuda(), C.c_int(-1)
        ctx.check(hip.lib.gh_potrf_solve_dev(ctx.h, C.c_void_p(dA.data_ptr()), n, lda, C.c_void_p(x.data_ptr()), C.byref(info)))
        ctx.sync()
        assert info.value == 0
        return x.cpu().numpy()

    x_step = solve("0", "0")
    for flow, chain in (("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")):
        x = solve(flow, chain)
        assert x.tobytes() == solve(flow, chain).tobytes()
        assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)
        assert np.abs(x - x_step).max() <= 1e-13 * np.abs(x_step).max()


@pytest.mark.parametrize("cams", [3, 11, 32, 50, 64, 100])
def test_ba_single_launch_factorisation_against_the_launch_path(ctx, cams, monkeypatch):
    """The right-hand-side row rides through the factorisation: inside the last diagonal tile (6 * cams not a multiple of
    64), or as a tile row of its own (cams = 32, 64: n = 192, 384)."""
    from gslam_amd import ba
    g = make_graph(cams, 40 * cams, n_obs_per_point=4, seed=cams)
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "1")
    p1, x1, s1, _ = ba.solve(ctx, g, ba.default_options(max_iterations=8, deterministic=1))
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "0")
    p0, x0, s0, _ = ba.solve(ctx, g, ba.default_options(max_iterations=8, deterministic=1))
    assert s1.iterations == s0.iterations and s1.accepted == s0.accepted
    assert abs(s1.final_cost - s0.final_cost) <= 1e-9 * abs(s0.final_cost)
    assert np.abs(p1 - p0).max() <= 1e-8 and np.abs(x1 - x0).max() <= 1e-8  # eight LM iterations amplify the rounding


@pytest.mark.parametrize("cams,points,per_point", [(12, 300, 5), (60, 6000, 6), (500, 50000, 6), (40, 3000, 12)])
def test_schur_pair_lists_built_on_the_gpu_equal_the_host_lists(ctx, cams, points, per_point, monkeypatch):
    """GSLAM_HIP_BA_PAIRS=check builds the deterministic Schur pair lists both ways and compares every table (pairs,
    block starts, block cameras, segment tables) element for element inside gh_ba_solve -- and the index lists built by
    the pool teams against the serial ones; the iterates must then equal the host-list run bit for bit."""
    from gslam_amd import ba
    g = make_graph(cams, points, n_obs_per_point=per_point, seed=cams + per_point)
    monkeypatch.setenv("GSLAM_HIP_BA_PAIRS", "host")
    p0, x0, s0, st0 = ba.solve(ctx, g, ba.default_options(max_iterations=4, deterministic=1))
    monkeypatch.setenv("GSLAM_HIP_BA_PAIRS", "check")
    p1, x1, s1, st1 = ba.solve(ctx, g, ba.default_options(max_iterations=4, deterministic=1))
    assert st0 == 0 and st1 == 0
    assert p1.tobytes() == p0.tobytes() and x1.tobytes() == x0.tobytes()
    monkeypatch.setenv("GSLAM_HIP_BA_PAIRS", "device")
    p2, x2, s2, st2 = ba.solve(ctx, g, ba.default_options(max_iterations=4, deterministic=1))
    assert st2 == 0 and p2.tobytes() == p0.tobytes() and x2.tobytes() == x0.tobytes()


def test_single_launch_kernels_give_up_instead_of_hanging(ctx, monkeypatch):
    """Every wait inside the single-launch factorisation / back-substitution is bounded.  With the bound shrunk to one poll
    the waits expire: the stand-alone solve reports it (info > n), and gh_ba_solve repeats the iteration on the
    launch-per-step path -- same iterates as with the single-launch kernels switched off."""
    from gslam_amd import ba
    n = 640
    rng = np.random.default_rng(5)
    M = rng.standard_normal((n, 96))
    A = M @ M.T / 96.0 + 2.0 * np.eye(n)
    g = make_graph(100, 4000, n_obs_per_point=4, seed=9)
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "0")
    monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", "0")
    p0, x0, s0, _ = ba.solve(ctx, g, ba.default_options(max_iterations=6, deterministic=1))
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "1")
    monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", "1")
    monkeypatch.setenv("GSLAM_HIP_FLOW_SPIN_LIMIT", "1")
    _, _, info = ba.potrf_solve(ctx, A, rng.standard_normal(n))
    assert info > n
    p1, x1, s1, _ = ba.solve(ctx, g, ba.default_options(max_iterations=6, deterministic=1))
    assert s1.iterations == s0.iterations and s1.accepted == s0.accepted
    assert p1.tobytes() == p0.tobytes() and x1.tobytes() == x0.tobytes()


def test_potrf_single_launch_reports_not_positive_definite(ctx, monkeypatch):
    from gslam_amd import ba
    monkeypatch.setenv("GSLAM_HIP_CHOL_FLOW", "1")
    A = np.eye(320)
    A[200, 200] = -1.0
    _, _, info = ba.potrf_solve(ctx, A, np.ones(320))
    assert info != 0


def test_potrf_reports_not_positive_definite(ctx):
    from gslam_amd import ba
    A = np.eye(100)
    A[70, 70] = -1.0
    _, _, info = ba.potrf_solve(ctx, A, np.ones(100))
    assert info != 0


def test_pnp_recovers_pose(ctx, oracle):
    from gslam_amd import ba
    g = make_graph(3, 200, n_obs_per_point=3, seed=11, noise=0.0, outlier_frac=0.0, perturb=False)
    sel = g["obs_cam"] == 1
    X = g["point_xyz_gt"][g["obs_point"][sel]]
    m = g["obs_xy"][sel]
    truth = g["cam_pose_gt"][1]
    start = oracle.se3_retract(truth, np.array([0.05, -0.04, 0.03, 0.01, -0.02, 0.015]))
    pose, s, info = ba.pnp(ctx, X, m, start, want_information=True)
    assert s.final_cost < 1e-20
    assert np.abs(pose - truth).max() < 1e-9 or np.abs(pose + np.r_[truth[:4], -truth[4:]] * 0 - truth).max() < 1e-9
    assert np.allclose(info, info.T) and np.all(np.linalg.eigvalsh(info) > 0)


@pytest.mark.parametrize("n", [8192, 16500, 33000, 60000])
def test_potrf_solve_large_residual_property(ctx, n):
    """Full-size property instead of an oracle: ||A x - b|| / ||b|| <= 1e-10 for a well conditioned SPD
    system; n = 16500 takes the 512-wide outer-panel path with ragged edge tiles, n = 33000 the 1024-wide one,
    n = 60000 is the full C5 reduced-camera system (28.8 GB; A and its factor = 57.6 GB of the 288 GB)."""
    import ctypes as C
    import torch
    from gslam_amd import hip
    g = torch.Generator(device="cuda").manual_seed(n)
    M = torch.randn((n, 256), dtype=torch.float64, device="cuda", generator=g)
    A = M @ M.T
    A /= 256.0
    A.diagonal().add_(4.0)  # in place: no second n x n temporary
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    L = A.clone()  # symmetric: row-major == column-major
    x = b.clone()
    info = C.c_int()
    ctx.check(hip.lib.gh_potrf_solve_dev(ctx.h, C.c_void_p(L.data_ptr()), n, n, C.c_void_p(x.data_ptr()), C.byref(info)))
    ctx.sync()
    assert info.value == 0
    r = torch.linalg.norm(A @ x - b) / torch.linalg.norm(b)
    assert float(r) <= 1e-10, float(r)
    if n > 20000:
        return  # the residual is the property; the O(n^3) reconstruction is checked at the smaller sizes
    # L L^T reproduces A on the lower triangle (column-major lower == row-major upper of the tensor)
    Lt = torch.triu(L)  # row-major view of the column-major lower factor is its transpose
    rec = Lt.T @ Lt
    assert float((rec - A).abs().max() / A.abs().max()) <= 1e-12


def test_resident_graph_equals_one_shot_solves(ctx, oracle):
    """gh_ba_graph_*: create once, then (a) a solve equals gh_ba_solve on the same problem bit for bit, (b) two solves of
    6 iterations continue where one of 12 would be (same trust-region restart aside: compared against the oracle run the
    same way), (c) new values through update() on the same topology equal a fresh one-shot solve of those values, and
    (d) a second graph on the same context does not disturb the first (own arenas)."""
    from gslam_amd import ba
    g = make_graph(20, 800, n_obs_per_point=5, seed=11)
    g["point_free"] = np.ones(800, np.uint8)
    g["point_free"][:7] = 0
    opts = ba.default_options(max_iterations=15)
    p1, x1, s1, st1 = ba.solve(ctx, g, opts)
    G = ba.Graph(ctx, g, opts)
    sg, stg = G.solve(opts)
    pg, xg = G.read()
    assert stg == st1 == 0 and sg.iterations == s1.iterations and sg.final_cost == s1.final_cost
    assert pg.tobytes() == p1.tobytes() and xg.tobytes() == x1.tobytes()
    # (c) new values, same topology: a noisier start
    rng = np.random.default_rng(3)
    g2 = dict(g)
    g2["cam_pose"] = g["cam_pose"].copy()
    g2["cam_pose"][1:, 4:] += rng.normal(size=(19, 3)) * 0.02
    g2["point_xyz"] = g["point_xyz"] + rng.normal(size=g["point_xyz"].shape) * 0.03
    g2["obs_xy"] = g["obs_xy"] + rng.normal(size=g["obs_xy"].shape) * 1e-4
    other = ba.Graph(ctx, make_graph(9, 200, n_obs_per_point=4, seed=5), opts)  # (d) a neighbour on the same context
    other.solve(opts)
    G.update(cam_pose=g2["cam_pose"], point_xyz=g2["point_xyz"], obs_xy=g2["obs_xy"])
    s2g, _ = G.solve(opts)
    p2g, x2g = G.read()
    p2, x2, s2, _ = ba.solve(ctx, g2, opts)
    assert s2g.iterations == s2.iterations and s2g.final_cost == s2.final_cost
    assert p2g.tobytes() == p2.tobytes() and x2g.tobytes() == x2.tobytes()
    eo = oracle.ba_solve(g2, oracle_lib.ba_options(max_iterations=15), threads=4)
    assert eo[2].iterations == s2g.iterations and np.abs(p2g - eo[0]).max() <= STATE_ATOL
    # (b) continuing on the resident state: 2 x 6 iterations from the original values == the oracle run the same way
    G.update(cam_pose=g["cam_pose"], point_xyz=g["point_xyz"], obs_xy=g["obs_xy"])
    o6 = ba.default_options(max_iterations=6)
    G.solve(o6)
    sB, _ = G.solve(o6)
    pB, xB = G.read()
    e1 = oracle.ba_solve(g, oracle_lib.ba_options(max_iterations=6), threads=4)
    gmid = dict(g)
    gmid["cam_pose"], gmid["point_xyz"] = e1[0], e1[1]
    e2 = oracle.ba_solve(gmid, oracle_lib.ba_options(max_iterations=6), threads=4)
    assert sB.iterations == e2[2].iterations and abs(sB.final_cost - e2[2].final_cost) <= COST_RTOL * e2[2].final_cost
    assert np.abs(pB - e2[0]).max() <= STATE_ATOL and np.abs(xB - e2[1]).max() <= STATE_ATOL
    other.close()
    G.close()


def test_resident_graph_c4_resolve_rate(ctx):
    """C4-sized graph kept on the device: re-solves skip the list building and the uploads."""
    import time
    from gslam_amd import ba
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1)
    opts = ba.default_options(max_iterations=12)
    ba.solve(ctx, g, opts)
    t0 = time.perf_counter()
    p1, x1, s1, _ = ba.solve(ctx, g, opts)
    t_one = time.perf_counter() - t0
    G = ba.Graph(ctx, g, opts)
    G.solve(opts)
    G.update(cam_pose=g["cam_pose"], point_xyz=g["point_xyz"])
    t0 = time.perf_counter()
    sg, _ = G.solve(opts)
    t_res = time.perf_counter() - t0
    pg, xg = G.read()
    assert sg.iterations == s1.iterations and pg.tobytes() == p1.tobytes() and xg.tobytes() == x1.tobytes()
    print(f"C4 one-shot {t_one * 1e3:.2f} ms, resident {t_res * 1e3:.2f} ms for {sg.iterations} iterations")
    assert t_res < t_one
    G.close()


@pytest.mark.parametrize("n,pad", [(20000, 0), (33000, 8)])
def test_blocked_cholesky_eight_wave_tiles_are_bit_identical(ctx, n, pad, monkeypatch):
    """Large systems: the trailing updates run with eight waves per 128 x 128 tile (four waves per SIMD).  Same sums per
    element: the factor and the solution must be the bits of the four-wave kernel's, and solve the system.
    pad > 0: the right-hand side rides as an extra row."""
    import ctypes as C
    import torch
    from gslam_amd import hip
    g = torch.Generator(device="cuda").manual_seed(n)
    M = torch.randn((n, 96), dtype=torch.float64, device="cuda", generator=g)
    lda = n + pad
    A = torch.zeros((n, lda), dtype=torch.float64, device="cuda")  # column-major n x n in an lda-row buffer = row-major (n, lda)
    A[:, :n] = M @ M.T / 96.0
    A[:, :n].diagonal().add_(2.0)
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GSLAM_HIP_SYRK8", mode)
        a, x = A.clone(), b.clone()
        info = C.c_int()
        ctx.check(hip.lib.gh_potrf_solve_dev(ctx.h, C.c_void_p(a.data_ptr()), n, lda, C.c_void_p(x.data_ptr()), C.byref(info)))
        ctx.sync()
        assert info.value == 0
        out[mode] = (torch.triu(a[:, :n]), x)  # (the buffer is the transpose: L^T sits in the upper triangle of the view)
    assert torch.equal(out["1"][0], out["0"][0]) and torch.equal(out["1"][1], out["0"][1])
    r = A[:, :n] @ out["1"][1] - b
    assert float(r.norm() / b.norm()) < 1e-11
    # in-panel updates two blocks at a time (rank 128) against one at a time: the same factor to rounding
    monkeypatch.setenv("GSLAM_HIP_CHOL_PAIR", "0")
    a, x = A.clone(), b.clone()
    info = C.c_int()
    ctx.check(hip.lib.gh_potrf_solve_dev(ctx.h, C.c_void_p(a.data_ptr()), n, lda, C.c_void_p(x.data_ptr()), C.byref(info)))
    ctx.sync()
    L0 = torch.triu(a[:, :n])
    assert info.value == 0 and float((L0 - out["1"][0]).abs().max()) <= 1e-12 * float(L0.abs().max())
    assert float((x - out["1"][1]).abs().max()) <= 1e-11 * float(x.abs().max())


@pytest.mark.parametrize("n", [8256, 8300, 16421])
def test_rhs_row_path_at_large_n_matches_the_plain_paths(ctx, n, monkeypatch):
    """gh_potrf_solve_dev with lda > n carries the right-hand side through the factorisation as row n of A (include/gslam_hip.h:
    the padding rows are scratch then).  Beyond n = 8192 the backward pass runs in segments, from n = 16384 the panels take
    blocks in pairs (rank-128 updates), n % 64 != 0 leaves a partial last block: each of these against the same call with
    GSLAM_HIP_CHOL_PAIR=0 / GSLAM_HIP_BWD_CHAIN=0 and against lda == n (forward + backward substitution after the
    factorisation), plus the residual property."""
    import ctypes as C
    import torch
    from gslam_amd import hip
    g = torch.Generator(device="cuda").manual_seed(n)
    M = torch.randn((n, 192), dtype=torch.float64, device="cuda", generator=g)
    A = M @ M.T
    A /= 192.0
    A.diagonal().add_(3.0)
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    lda = (n + 1 + 15) // 16 * 16

    def solve(with_row):
        ld = lda if with_row else n
        buf = torch.zeros((n, ld), dtype=torch.float64, device="cuda")  # column-major n x n inside ld-row columns
        buf[:, :n] = A  # symmetric: column j of the column-major matrix = row j of the tensor
        x = b.clone()
        info = C.c_int()
        ctx.check(hip.lib.gh_potrf_solve_dev(ctx.h, C.c_void_p(buf.data_ptr()), n, ld, C.c_void_p(x.data_ptr()), C.byref(info)))
        ctx.sync()
        assert info.value == 0
        return x, buf[:, :n].clone()

    x_row, L_row = solve(True)
    assert float(torch.linalg.norm(A @ x_row - b) / torch.linalg.norm(b)) <= 1e-11
    x_plain, L_plain = solve(False)
    assert float((torch.triu(L_row) - torch.triu(L_plain)).abs().max()) == 0.0  # the factor does not depend on who carries b
    assert float((x_row - x_plain).abs().max() / x_plain.abs().max()) <= 1e-12
    monkeypatch.setenv("GSLAM_HIP_CHOL_PAIR", "0")
    monkeypatch.setenv("GSLAM_HIP_BWD_CHAIN", "0")
    x_ref, L_ref = solve(True)
    assert float((torch.triu(L_row) - torch.triu(L_ref)).abs().max() / torch.triu(L_ref).abs().max()) <= 1e-12
    assert float((x_row - x_ref).abs().max() / x_ref.abs().max()) <= 1e-12
