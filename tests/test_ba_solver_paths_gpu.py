"""The newest ways gh_ba_solve reaches its answer, pinned to references instead of to the GPU's own other path:

  reordered cameras  shuffled graphs renumbered by ba_order.hip, rebuilt in that order (ArrowProblem) and handed back in the
                     caller's order, against the ORACLE on the shuffled graph (tests/test_ba_order_gpu.py compares them with the
                     GPU's in-order solve only);
  wide borders       co-visibility windows of 31 / 32 / 33 cameras: shuffled, they come back as a band + a border of 81 / 207
                     cameras (486 / 1242 border rows); in order, window 32 is the widest band the solver takes (half-bandwidth 191)
                     and window 33 goes to the dense factorisation;
  n >= 65 536        the compact columns (cr_map.h) with 7 .. 9 fill slots against scipy's banded Cholesky, and a 12 000-camera BA
                     (n = 72 000) through the band solver and through the dense one.

Bars of tests/ba_parity.py: identical accept / reject sequence, cost 1e-9, state 1e-8.  The oracle does not read the GSLAM_HIP_BA_*
switches, so it runs once per (graph, iterations) and every solver variant of that graph shares the run."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
from ba_parity import COST_RTOL, STATE_ATOL_FULL, _compare_ba
from gslam_amd.ba_synth import make_graph
from lm_trace import assert_identical_trace, assert_same_trace
from test_ba_order import _shuffle

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


@functools.lru_cache(maxsize=None)
def _graph(cams, points, seed, closures=0, window=None, shuffled=False):
    g = make_graph(cams, points, n_obs_per_point=6, seed=seed, loop_closures=closures, covis_window=window)
    return _shuffle(g, seed)[0] if shuffled else g


_ORACLE = {}


def _oracle_run(oracle, key, max_it):
    """the oracle's (poses, points, summary, status) for _graph(*key) at max_it iterations, Huber 0.01: once per module"""
    if (key, max_it) not in _ORACLE:
        _ORACLE[(key, max_it)] = oracle.ba_solve(_graph(*key), oracle_lib.ba_options(huber=0.01, max_iterations=max_it),
                                                 threads=THREADS)
    return _ORACLE[(key, max_it)]


def _vs_oracle(oracle, ctx, key, max_it):
    return _compare_ba(oracle, ctx, _graph(*key), max_it, eo=_oracle_run(oracle, key, max_it))


# ---------------------------------------------------------------------------------------------------- reordered cameras

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shuffled_c4_band_vs_oracle(ctx, oracle, seed):
    key = (500, 50000, seed, 0, None, True)
    so = _vs_oracle(oracle, ctx, key, 40)
    assert ctx.last_ba_solver()[0] == "band" and ctx.last_ba_order() == (0, True)
    assert so.termination == 1 and so.final_cost < 0.5 * so.initial_cost


@pytest.mark.parametrize("border", ["cameras", "points", "auto"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shuffled_c4_loop_closures_vs_oracle(ctx, oracle, monkeypatch, seed, border):
    if border != "auto":
        monkeypatch.setenv("GSLAM_HIP_BA_POINT_BORDER", "1" if border == "points" else "0")
    key = (500, 50000, seed, 20, None, True)
    _vs_oracle(oracle, ctx, key, 40)
    assert ctx.last_ba_solver()[0] == "arrow" and ctx.last_ba_order()[1]
    assert ctx.last_ba_border_points() == (0 if border == "cameras" else 20)
    assert (ctx.last_ba_order()[0] > 0) == (border == "cameras")


# C5/10 to convergence, not the 12 iterations of test_full_configs_gpu.py: after 12 (all accepted, not converged) the ORACLE on the
# shuffled graph lies 2.6e-8 (4.4e-8 with the closures) in pose from the oracle on the in-order graph -- rounding alone moves an
# unconverged state past the 1e-8 bar.  Converged (22 iterations) the two oracle runs agree to 1.3e-10 / 2.4e-10 in pose and
# 1.6e-10 / 3.3e-10 in points, as at C4 (test_ba_oracle.py::test_full_c4_oracle_camera_order_sensitivity).
def test_shuffled_c5_tenth_band_vs_oracle(ctx, oracle):
    so = _vs_oracle(oracle, ctx, (1000, 100000, 1, 0, None, True), 40)
    assert ctx.last_ba_solver()[0] == "band" and ctx.last_ba_order() == (0, True)
    assert so.termination == 1


@pytest.mark.parametrize("border", ["cameras", "points"])
def test_shuffled_c5_tenth_loop_closures_vs_oracle(ctx, oracle, monkeypatch, border):
    monkeypatch.setenv("GSLAM_HIP_BA_POINT_BORDER", "1" if border == "points" else "0")
    so = _vs_oracle(oracle, ctx, (1000, 100000, 1, 10, None, True), 40)
    assert so.termination == 1
    assert ctx.last_ba_solver()[0] == "arrow" and ctx.last_ba_order()[1]
    assert ctx.last_ba_border_points() == (10 if border == "points" else 0)


@pytest.mark.parametrize("border", ["cameras", "points"])
def test_shuffled_c4_loop_closures_atomics_vs_oracle(ctx, oracle, monkeypatch, border):
    """deterministic = 0 (f64 atomics in the assembly) on the reordered arrowhead: lm_trace.assert_same_trace, as
    test_ba_gpu._compare holds the atomics mode; the states at 1e-8 when the two traces come out identical."""
    from gslam_amd import ba
    monkeypatch.setenv("GSLAM_HIP_BA_POINT_BORDER", "1" if border == "points" else "0")
    key = (500, 50000, 1, 20, None, True)
    g, eo = _graph(*key), _oracle_run(oracle, key, 40)
    poses, pts, sg, st = ba.solve(ctx, g, ba.default_options(huber_delta=0.01, max_iterations=40, deterministic=0))
    assert st == 0 and ctx.last_ba_solver()[0] == "arrow" and ctx.last_ba_order()[1]
    assert ctx.last_ba_border_points() == (20 if border == "points" else 0)
    if assert_same_trace(sg, eo[2]):
        assert np.abs(poses - eo[0]).max() <= STATE_ATOL_FULL and np.abs(pts - eo[1]).max() <= STATE_ATOL_FULL
    assert abs(oracle.ba_cost(g, poses, pts) - sg.final_cost) <= 1e-12 * sg.final_cost


# ---------------------------------------------------------------------------------------------------- wide borders

WIDE = [(31, True, "arrow", "0"), (31, True, "arrow", "1"), (32, True, "arrow", "0"), (32, True, "arrow", "1"),
        (32, False, "band", None), (33, False, "dense", None), (33, True, "dense", None)]


@pytest.mark.parametrize("window,shuffled,route,dense_border", WIDE)
def test_wide_window_vs_oracle(ctx, oracle, monkeypatch, window, shuffled, route, dense_border):
    """GSLAM_HIP_BA_ARROW_DENSE_BORDER = 0: the border kernels skip the blocks the host-side propagation marks zero; = 1: every
    block dense (1242 border rows x ~3000 unknowns lies near the 4 M-entry default threshold).  Only the arrowhead reads it."""
    from gslam_amd import ba
    if dense_border is not None:
        monkeypatch.setenv("GSLAM_HIP_BA_ARROW_DENSE_BORDER", dense_border)
    key = (500, 50000, 1, 0, window, shuffled)
    _, nb, span, re = ba.camera_order(_graph(*key))
    _vs_oracle(oracle, ctx, key, 40)
    used, order = ctx.last_ba_solver(), ctx.last_ba_order()
    print("window %d %s: route %s, tiles %d, span %d, border cameras %d" % (window, "shuffled" if shuffled else "in order", used[0],
                                                                            used[1], used[2], order[0]))
    assert used[0] == route
    assert order == (nb, re) and ctx.last_ba_border_points() == 0
    if route == "arrow":
        assert nb > 0 and used[2] == span <= 31
    if route == "band":
        assert used[1:] == (3, 31) and order == (0, False)


def test_wide_window_shuffled_resident_graph_vs_oracle(ctx, oracle):
    """gh_ba_graph_create / _solve / _update / _solve / _read on the shuffled window-32 graph (207 border cameras): bitwise the
    one-shot solve, and within the oracle's bars."""
    from gslam_amd import ba
    key = (500, 50000, 1, 0, 32, True)
    h, eo = _graph(*key), _oracle_run(oracle, key, 40)
    opts = ba.default_options(huber_delta=0.01, max_iterations=40, deterministic=1)
    p1, x1, s1, st = ba.solve(ctx, h, opts)
    assert st == 0 and ctx.last_ba_solver()[0] == "arrow"
    G = ba.Graph(ctx, h, opts)
    try:
        for attempt in range(2):
            if attempt:
                G.update(cam_pose=h["cam_pose"], point_xyz=h["point_xyz"], cam_dof=h["cam_dof"])
            s2, st2 = G.solve(opts)
            assert st2 == 0 and ctx.last_ba_solver()[0] == "arrow" and ctx.last_ba_order()[0] > 0
            assert (s2.iterations, s2.final_cost) == (s1.iterations, s1.final_cost)
            p2, x2 = G.read()
            assert np.array_equal(p2, p1) and np.array_equal(x2, x1)
            assert_identical_trace(s2, eo[2], rtol=COST_RTOL)
            assert np.abs(p2 - eo[0]).max() <= STATE_ATOL_FULL and np.abs(x2 - eo[1]).max() <= STATE_ATOL_FULL
    finally:
        G.close()


# ---------------------------------------------------------------------------------------------------- n >= 65 536, compact

def _band_spd(n, hb, seed, border=None):
    """A well-conditioned SPD band in LAPACK lower-band storage (ab[i, c] = A[c + i, c]) and an optional dense border
    (E: nbr x n band rows, C: nbr x nbr symmetric) -- never an n x n array.  Diagonal = largest absolute row sum + 1, as
    test_cr_solver.make_band / make_arrow."""
    rng = np.random.default_rng(seed)
    ab = rng.standard_normal((hb + 1, n))
    for i in range(1, hb + 1):
        ab[i, n - i:] = 0.0
    ab[0] *= 2.0  # (A + A^T on the diagonal)
    rows = np.abs(ab[0]).copy()
    for i in range(1, hb + 1):
        rows[i:] += np.abs(ab[i, :n - i])
        rows[:n - i] += np.abs(ab[i, :n - i])
    E = C = None
    if border:
        nbr, fill = border
        E = rng.standard_normal((nbr, n)) * (rng.random((nbr, n)) < fill)
        C = np.tril(rng.standard_normal((nbr, nbr)))
        C = C + C.T
        rows += np.abs(E).sum(0)
        crow = np.abs(E).sum(1) + np.abs(C).sum(1)
        boost = max(rows.max(), crow.max()) + 1.0
        C += np.eye(nbr) * boost
    else:
        boost = rows.max() + 1.0
    ab[0] += boost
    return ab, E, C


def _compact_columns(ab, E, C, n_band, lda, m, brow):
    """The compact columns of include/gslam_hip.h (gh_cr_compact_layout) straight from the band storage: band element
    (c + i, c) at local row c - J m + i (J = c / m), border row k at brow + k; fill slots stay zero."""
    hb = ab.shape[0] - 1
    nbr = 0 if E is None else E.shape[0]
    buf = np.zeros((n_band + nbr, lda))
    c = np.arange(n_band)
    for i in range(hb + 1):
        cc = c[:n_band - i]
        buf[cc, cc % m + i] = ab[i, :n_band - i]
    if nbr:
        buf[:n_band, brow:brow + nbr] = E.T
        for k in range(nbr):
            buf[n_band + k, brow + k:brow + nbr] = C[k:, k]
    return buf


def _band_matvec(ab, E, C, x):
    n = ab.shape[1]
    xb = x[:n]
    y = ab[0] * xb
    for i in range(1, ab.shape[0]):
        y[i:] += ab[i, :n - i] * xb[:n - i]
        y[:n - i] += ab[i, :n - i] * xb[i:]
    if E is None:
        return y
    xe = x[n:]
    return np.concatenate([y + E.T @ xe, E @ xb + C @ xe])


def _reference(ab, E, C, b):
    """scipy's banded Cholesky; with a border, the Schur complement C - E B^-1 E^T through it and a dense Cholesky"""
    from scipy.linalg import cho_factor, cho_solve, solveh_banded
    n = ab.shape[1]
    if E is None:
        return solveh_banded(ab, b, lower=True)
    Z = solveh_banded(ab, np.concatenate([b[:n, None], E.T], axis=1), lower=True)
    y, Z = Z[:, 0], Z[:, 1:]
    x2 = cho_solve(cho_factor(C - E @ Z, lower=True), b[n:] - E @ y)
    return np.concatenate([y - Z @ x2, x2])


@pytest.mark.parametrize("n_band,hb,nbr,slots", [(65535, 191, 0, 8), (65536, 191, 0, 8), (65537, 191, 0, 8), (120000, 185, 0, 9),
                                                 (120000, 149, 0, 9), (72000, 191, 129, 7)])
def test_compact_solve_past_65536_vs_scipy(ctx, n_band, hb, nbr, slots):
    """gh_arrow_solve_compact_dev past 2^16 unknowns, with up to 9 fill slots (test_cr_solver.py stops at n = 6000, 5 slots)"""
    from gslam_amd import ba
    lda, m, brow = ba.compact_layout(n_band, hb, nbr)
    assert brow == (2 + slots) * m, "fill slots of the layout"
    ab, E, C = _band_spd(n_band, hb, seed=n_band + hb + nbr, border=(nbr, 0.05) if nbr else None)
    b = np.random.default_rng(7).standard_normal(n_band + nbr)
    cols = _compact_columns(ab, E, C, n_band, lda, m, brow)
    x, info = ba.arrow_solve_compact_columns(ctx, cols, b, n_band, hb)
    assert info == 0
    xr = _reference(ab, E, C, b)
    err = np.abs(x - xr).max() / np.abs(xr).max()
    res = np.abs(_band_matvec(ab, E, C, x) - b).max() / np.abs(b).max()
    print("n_band %d hb %d nbr %d: |x - x_ref| / |x_ref| %.2g, residual %.2g" % (n_band, hb, nbr, err, res))
    assert err <= 1e-12
    assert res <= 1e-10
    x2, info2 = ba.arrow_solve_compact_columns(ctx, cols, b, n_band, hb)
    assert info2 == 0 and x2.tobytes() == x.tobytes(), "fixed summation order: two runs agree bit for bit"


# ---------------------------------------------------------------------------------------------------- n >= 65 536, BA

def test_12k_cameras_band_and_dense_agree_past_65536(ctx, oracle):
    """12 000 cameras / 1.2 M points (n = 72 000): the band solver (auto) and the dense factorisation (41 GB lower triangle) run
    the same LM iteration; each returned state has the oracle's cost its summary reports."""
    import torch
    from gslam_amd import ba
    g = make_graph(12000, 1200000, n_obs_per_point=6, seed=1)
    opts = ba.default_options(huber_delta=0.01, max_iterations=3, deterministic=1)
    runs = {}
    for solver in ("auto", "dense"):
        ctx.trim()
        torch.cuda.empty_cache()
        ctx.set_ba_solver(solver)
        try:
            poses, pts, s, st = ba.solve(ctx, g, opts)
            used = ctx.last_ba_solver()[0]
        finally:
            ctx.set_ba_solver("auto")
            ctx.trim()
            torch.cuda.empty_cache()
        assert st == 0 and used == ("band" if solver == "auto" else "dense")
        assert np.isfinite(poses).all() and np.isfinite(pts).all()
        assert abs(oracle.ba_cost(g) - s.initial_cost) <= 1e-12 * s.initial_cost
        assert abs(oracle.ba_cost(g, poses, pts) - s.final_cost) <= 1e-12 * s.final_cost
        runs[solver] = (poses, pts, s)
    (pb, xb, sb), (pd, xd, sd) = runs["auto"], runs["dense"]
    assert sb.iterations == 3 and sb.accepted >= 2
    assert_identical_trace(sd, sb, rtol=COST_RTOL)
    assert np.abs(pd - pb).max() <= STATE_ATOL_FULL and np.abs(xd - xb).max() <= STATE_ATOL_FULL
