"""The solver's own camera order (gslam_amd/csrc/ba_order.hip, gh_ba_camera_order): host code, runs without a GPU.

GSLAM::BundleGraph::keyframes is a plain vector (GSLAM/core/Optimizer.h:116-119,150-157); the band / arrowhead solvers must not
depend on the order a caller happens to fill it in (VERDICT r5 missing #2).  Here: trajectories handed over in temporal order
keep their order; the same graphs with the cameras SHUFFLED come back as a band (or band + border) whose span fits the solver;
graphs that are no band in any order are left alone."""
import numpy as np
import pytest

from gslam_amd.ba_synth import make_graph

BAND_SPAN = 31  # 6 * 31 + 5 = 191 <= 3 * 64 (chol_cr.hip: gh_cr_tiles)


def _shuffle(g, seed):
    """the same graph with the cameras renumbered by a random permutation (and the observation list shuffled too)"""
    rng = np.random.default_rng(seed)
    nc = len(g["cam_dof"])
    new_of_old = rng.permutation(nc).astype(np.int32)
    old_of_new = np.argsort(new_of_old)
    h = dict(g)
    h["cam_pose"] = g["cam_pose"][old_of_new]
    h["cam_dof"] = g["cam_dof"][old_of_new]
    for k in ("cam_pose_gt",):
        if k in g:
            h[k] = g[k][old_of_new]
    oo = rng.permutation(len(g["obs_cam"]))
    h["obs_cam"] = new_of_old[g["obs_cam"]][oo].astype(np.int32)
    h["obs_point"] = np.asarray(g["obs_point"])[oo]
    h["obs_xy"] = np.asarray(g["obs_xy"])[oo]
    return h, new_of_old


def _span(g, perm, n_border):
    pos = np.empty(len(perm), np.int64)
    pos[perm] = np.arange(len(perm))
    c = pos[g["obs_cam"]]
    keep = c < len(perm) - n_border
    p = np.asarray(g["obs_point"])[keep]
    c = c[keep]
    lo = np.full(len(g["point_xyz"]), 1 << 30)
    hi = np.full(len(g["point_xyz"]), -1)
    np.minimum.at(lo, p, c)
    np.maximum.at(hi, p, c)
    seen = hi >= 0
    return int((hi[seen] - lo[seen]).max())


def test_trajectory_in_order_is_left_alone():
    from gslam_amd import ba
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1)
    perm, nb, span, re = ba.camera_order(g)
    assert np.array_equal(perm, np.arange(500)) and nb == 0 and not re and span == _span(g, perm, 0) <= 24


def test_loop_closures_in_order_take_the_round5_arrow_order():
    from gslam_amd import ba
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1, loop_closures=20)
    perm, nb, span, re = ba.camera_order(g)
    assert not re and 0 < nb <= 120 and span <= BAND_SPAN and sorted(perm) == list(range(500))
    assert np.all(np.diff(perm[:500 - nb]) > 0) and np.all(np.diff(perm[500 - nb:]) > 0)  # compact renumbering, order kept
    assert span == _span(g, perm, nb)


@pytest.mark.parametrize("cams,points,seed", [(500, 50000, 1), (500, 50000, 2), (500, 50000, 3), (160, 8000, 4), (1000, 100000, 5),
                                              (2000, 40000, 6)])
def test_shuffled_trajectory_comes_back_as_a_band(cams, points, seed):
    from gslam_amd import ba
    g = make_graph(cams, points, n_obs_per_point=6, seed=seed)
    h, _ = _shuffle(g, seed)
    perm, nb, span, re = ba.camera_order(h)
    assert re and nb == 0 and sorted(perm) == list(range(cams))
    assert span == _span(h, perm, 0)
    assert span <= BAND_SPAN, span


@pytest.mark.parametrize("cams,points,closures,span_c,seed", [(500, 50000, 20, None, 1), (500, 50000, 20, None, 2), (500, 50000, 20, None, 3),
                                                              (300, 20000, 12, None, 4), (2000, 200000, 30, 1000, 5)])
def test_shuffled_loop_closure_graph_comes_back_as_band_plus_border(cams, points, closures, span_c, seed):
    from gslam_amd import ba
    g = make_graph(cams, points, n_obs_per_point=6, seed=seed, loop_closures=closures, closure_span=span_c)
    _, nb0, _, _ = ba.camera_order(g)
    h, _ = _shuffle(g, seed)
    perm, nb, span, re = ba.camera_order(h)
    assert re and sorted(perm) == list(range(cams))
    assert 0 < nb <= 2 * nb0 + 8, (nb, nb0)   # about the border of the in-order graph
    assert span == _span(h, perm, nb) <= BAND_SPAN


def test_c5_shuffled_order_and_its_cost():
    """10 k cameras / 1 M points / 6 M observations, shuffled: a band again; the ordering is sampled (<= 2^20 observations) so its
    cost stays a small part of a one-shot solve (printed: the box this runs on decides the number)."""
    import time
    from gslam_amd import ba
    g = make_graph(10000, 1000000, n_obs_per_point=6, seed=1)
    h, _ = _shuffle(g, 1)
    t0 = time.perf_counter()
    perm, nb, span, re = ba.camera_order(h)
    dt = time.perf_counter() - t0
    print("C5 shuffled: camera order in %.1f ms (span %d)" % (dt * 1e3, span))
    assert re and nb == 0 and span <= BAND_SPAN, (nb, span)
    t0 = time.perf_counter()
    perm0, nb0, span0, re0 = ba.camera_order(g)
    print("C5 in order: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    assert not re0 and nb0 == 0 and span0 <= 24


def test_graph_that_is_no_band_is_left_alone_or_improved():
    """every point seen from cameras drawn over the WHOLE trajectory: no order makes this a band -> no border, dense path"""
    from gslam_amd import ba
    rng = np.random.default_rng(9)
    g = make_graph(300, 6000, n_obs_per_point=6, seed=9)
    g["obs_cam"] = rng.integers(0, 300, size=len(g["obs_cam"])).astype(np.int32)
    perm, nb, span, re = ba.camera_order(g)
    assert nb == 0 and sorted(perm) == list(range(300)) and span > BAND_SPAN


def test_two_disconnected_trajectories_and_unobserved_cameras():
    from gslam_amd import ba
    a = make_graph(300, 20000, n_obs_per_point=6, seed=11)
    nc = 700  # cameras 0..299: trajectory A, 300..399 unobserved, 400..699: trajectory B
    g = dict(a)
    g["cam_dof"] = np.full(nc, 63, np.int32)
    g["cam_pose"] = np.tile(a["cam_pose"][0], (nc, 1))
    g.pop("cam_pose_gt", None)
    g["obs_cam"] = np.concatenate([a["obs_cam"], a["obs_cam"] + 400]).astype(np.int32)
    g["obs_point"] = np.concatenate([a["obs_point"], a["obs_point"] + len(a["point_xyz"])]).astype(np.int32)
    g["obs_xy"] = np.concatenate([a["obs_xy"], a["obs_xy"]])
    g["point_xyz"] = np.concatenate([a["point_xyz"], a["point_xyz"]])
    h, _ = _shuffle(g, 12)
    perm, nb, span, re = ba.camera_order(h)
    assert re and nb == 0 and sorted(perm) == list(range(nc)) and span <= BAND_SPAN


def test_bad_indices_are_refused():
    from gslam_amd import ba
    g = make_graph(200, 5000, n_obs_per_point=6, seed=13)
    g["obs_cam"] = g["obs_cam"].copy()
    g["obs_cam"][7] = 200
    with pytest.raises(ValueError):
        ba.camera_order(g)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("window", [31, 32, 33])
def test_wide_covisibility_windows_around_the_band_limit(window, shuffled):
    """Co-visibility windows of 31 / 32 / 33 cameras (in-order span 30 / 31 / 32): the widest band the solver takes (window 32,
    span 31: half-bandwidth 6 * 31 + 5 = 191), and one past it.  What the ordering returns today; the border it finds for the
    shuffled graphs (printed) decides speed, not correctness, so it carries no bound here."""
    from gslam_amd import ba
    g = make_graph(500, 50000, n_obs_per_point=6, seed=1, covis_window=window)
    h = _shuffle(g, 1)[0] if shuffled else g
    perm, nb, span, re = ba.camera_order(h)
    print("window %d %s: border cameras %d, span %d, reordered %s" % (window, "shuffled" if shuffled else "in order", nb, span, re))
    assert np.array_equal(np.sort(perm), np.arange(500))
    assert span == _span(h, perm, nb)
    if nb > 0 or re:
        assert span <= BAND_SPAN
    if window == 32 and not shuffled:
        assert nb == 0 and span == BAND_SPAN and not re and np.array_equal(perm, np.arange(500))
    if window == 33:
        assert nb == 0 and not re and span > BAND_SPAN


@pytest.mark.parametrize("cams,points", [(60, 3000), (500, 50000), (10000, 1000000)])
@pytest.mark.parametrize("seed", [1, 2])
def test_covis_window_default_draws_the_same_graph(cams, points, seed):
    """make_graph(covis_window=25) is the default window: every existing graph byte for byte (the 1 M-point C5 graph crosses the
    2^18-point chunk of _pick_observers)."""
    a = make_graph(cams, points, n_obs_per_point=6, seed=seed)
    b = make_graph(cams, points, n_obs_per_point=6, seed=seed, covis_window=25)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
