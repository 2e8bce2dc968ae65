"""GPU parity of gh_triangulate_tracks_dev with the scalar restatement tests/tracks_restate.py, byte for byte, on the census
inputs of tests/tracks_cases.py (tests/test_tracks_cpu.py shows what they reach) and on a 40-camera / 2000-point graph with
noise and outliers; then the call in its place, between registered cameras and gh_ba_solve.  Output buffers go in filled with
0xAB (7.0 for doubles, -5 for ints)."""
import ctypes as C

import numpy as np
import pytest

import tracks_cases as tc
import tracks_restate as tr

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS = ("point_xyz", "status", "n_good", "obs_good")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(**kw):
    from gslam_amd import estimator
    p = estimator.track_default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _dirty(n_points, n_obs):
    import torch
    return dict(point_xyz=torch.full((max(n_points, 1), 3), tc.FILL_XYZ, dtype=torch.float64, device="cuda"),
                status=torch.full((max(n_points, 1),), tc.FILL_INT, dtype=torch.int32, device="cuda"),
                n_good=torch.full((max(n_points, 1),), tc.FILL_INT, dtype=torch.int32, device="cuda"),
                obs_good=torch.full((max(n_obs, 1),), tc.FILL_BYTE, dtype=torch.uint8, device="cuda"))


def _untouched(out):
    return ((out["point_xyz"] == tc.FILL_XYZ).all().item() and (out["status"] == tc.FILL_INT).all().item() and
            (out["n_good"] == tc.FILL_INT).all().item() and (out["obs_good"] == tc.FILL_BYTE).all().item())


def _run(ctx, a, params, use_masks=True, n_obs=None, n_points=None, expect=0):
    """gh_triangulate_tracks_dev on dirty output buffers -> dict of host arrays (cut to the sizes of the call)."""
    import torch
    from gslam_amd import hip
    n_obs = len(a["obs_cam"]) if n_obs is None else n_obs
    n_points = a["n_points"] if n_points is None else n_points
    d = {k: _dev(a[k]) for k in ("cam_pose", "obs_cam", "obs_point", "obs_xy")}
    use = _dev(a["obs_use"]) if use_masks and a.get("obs_use") is not None else None
    sel = _dev(a["point_select"]) if use_masks and a.get("point_select") is not None else None
    out = _dirty(n_points, n_obs)
    prm = _params(**params)
    st = hip.lib.gh_triangulate_tracks_dev(ctx.h, _ptr(d["cam_pose"]), len(a["cam_pose"]), _ptr(d["obs_cam"]), _ptr(d["obs_point"]),
                                           _ptr(d["obs_xy"]), n_obs, n_points, _ptr(use), _ptr(sel), C.byref(prm),
                                           *(_ptr(out[k]) for k in OUTPUTS))
    assert st == expect, (st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    if n_points == 0 or expect != 0:
        assert _untouched(out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got["point_xyz"][n_points:] == tc.FILL_XYZ).all() and (got["obs_good"][n_obs:] == tc.FILL_BYTE).all()
    return {k: got[k][:(n_obs if k == "obs_good" else n_points)] for k in OUTPUTS}


def _want(e):
    return dict(point_xyz=np.array(e["point_xyz"], np.float64).reshape(-1, 3), status=np.array(e["status"], np.int32),
                n_good=np.array(e["n_good"], np.int32), obs_good=np.array(e["obs_good"], np.uint8))


def _assert_same(got, want, names, tracks):
    for p in range(len(want["status"])):  # per point first: a failure names the case
        name = names[p] if names else p
        assert got["status"][p] == want["status"][p], (name, got["status"][p], want["status"][p], got["n_good"][p], want["n_good"][p])
        assert got["n_good"][p] == want["n_good"][p], (name, got["n_good"][p], want["n_good"][p])
        assert got["obs_good"][tracks[p]].tolist() == want["obs_good"][tracks[p]].tolist(), name
        assert got["point_xyz"][p].tobytes() == want["point_xyz"][p].tobytes(), (name, got["point_xyz"][p], want["point_xyz"][p])
    for k in OUTPUTS:  # then everything, the observations nobody owns included
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_census_matches_the_restatement_bit_for_bit(ctx):
    a, e = tc.arrays(), tc.expected()
    got = _run(ctx, a, tc.PARAMS)
    _assert_same(got, _want(e), a["names"], e["tracks"])
    skipped = got["status"] == tr.SKIPPED
    assert skipped.sum() == 2 and (got["point_xyz"][skipped] == tc.FILL_XYZ).all()  # not written: the caller's values survive
    assert set(got["status"].tolist()) == {0, 1, 2, 3, 4, 5} and got["obs_good"].sum() > 700


def test_noisy_graph_matches_the_restatement_bit_for_bit(ctx):
    g, e = tc.graph(True), tc.graph_expected(True)
    a = dict(g, n_points=len(g["point_xyz"]))
    got = _run(ctx, a, tc.GRAPH_PARAMS[True], use_masks=False)
    _assert_same(got, _want(e), None, e["tracks"])
    assert (got["status"] == tr.OK).sum() >= 1980 and (got["n_good"] == 4).sum() > 10  # the rounds ran on the device too


def test_exact_graph_matches_the_restatement_bit_for_bit(ctx):
    g, e = tc.graph(False), tc.graph_expected(False)
    got = _run(ctx, dict(g, n_points=len(g["point_xyz"])), tc.GRAPH_PARAMS[False], use_masks=False)
    _assert_same(got, _want(e), None, e["tracks"])
    assert (got["status"] == tr.OK).all() and np.abs(got["point_xyz"] - g["point_xyz_gt"]).max() < 1e-9


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    a = tc.arrays()
    one, two = _run(ctx, a, tc.PARAMS), _run(ctx, a, tc.PARAMS)
    for k in OUTPUTS:
        assert one[k].tobytes() == two[k].tobytes(), k


def test_without_observations_and_without_points(ctx):
    a = dict(tc.arrays())
    a["point_select"] = np.array([1, 1, 0, 1, 1], np.uint8)
    got = _run(ctx, a, tc.PARAMS, n_obs=0, n_points=5)
    assert got["status"].tolist() == [tr.TOO_FEW, tr.TOO_FEW, tr.SKIPPED, tr.TOO_FEW, tr.TOO_FEW]
    assert not got["n_good"].any()
    assert got["point_xyz"].tolist() == [[0.0] * 3, [0.0] * 3, [tc.FILL_XYZ] * 3, [0.0] * 3, [0.0] * 3]
    got = _run(ctx, a, tc.PARAMS, n_points=0)  # GH_OK, nothing launched: _run has checked that every buffer is as it was
    assert len(got["status"]) == 0


def test_argument_errors_leave_the_outputs_alone(ctx):
    from gslam_amd import hip
    a = tc.arrays()
    d = {k: _dev(a[k]) for k in ("cam_pose", "obs_cam", "obs_point", "obs_xy")}
    n_cams, n_obs, n_points = len(a["cam_pose"]), len(a["obs_cam"]), a["n_points"]
    out = _dirty(n_points, n_obs)
    nan = float("nan")

    def call(ctx_h=ctx.h, params=tc.PARAMS, sizes=(n_cams, n_obs, n_points), null=None):
        prm = None if params is None else C.byref(_params(**params))
        ptr = {k: (None if k == null else _ptr(t)) for k, t in list(d.items()) + list(out.items())}
        return hip.lib.gh_triangulate_tracks_dev(ctx_h, ptr["cam_pose"], sizes[0], ptr["obs_cam"], ptr["obs_point"], ptr["obs_xy"],
                                                 sizes[1], sizes[2], None, None, prm, *(ptr[k] for k in OUTPUTS))

    assert call(ctx_h=None) == GH_ERR_ARG
    assert call(params=None) == GH_ERR_ARG
    for k in ("cam_pose", "obs_cam", "obs_point", "obs_xy") + OUTPUTS:
        assert call(null=k) == GH_ERR_ARG, k
    for sizes in ((-1, n_obs, n_points), (n_cams, -1, n_points), (n_cams, n_obs, -1)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for bad in (dict(min_parallax_cos=0.0), dict(min_parallax_cos=-0.5), dict(min_parallax_cos=1.0000001), dict(min_parallax_cos=nan),
                dict(max_reproj=-1e-3), dict(max_reproj=nan), dict(min_views=1), dict(min_views=0), dict(min_views=-3),
                dict(max_drops=-1)):
        assert call(params=dict(tc.PARAMS, **bad)) == GH_ERR_ARG, bad
    ctx.sync()
    assert _untouched(out)
    # the ends of the allowed ranges are accepted
    assert call(params=dict(tc.PARAMS, min_parallax_cos=1.0, max_reproj=0.0, max_drops=0)) == 0
    ctx.sync()
    assert not _untouched(out)


def test_another_interleaving_gives_the_same_points(ctx):
    a, e = tc.arrays(), tc.expected()
    b, perm = tc.permuted(a, seed=4)
    one, two = _run(ctx, a, tc.PARAMS), _run(ctx, b, tc.PARAMS)
    for k in ("point_xyz", "status", "n_good"):
        assert one[k].tobytes() == two[k].tobytes(), k
    assert np.array_equal(two["obs_good"], one["obs_good"][perm])
    # grouped by point, ascending: what a caller with sorted arrays passes
    order = np.argsort(np.where((a["obs_point"] >= 0) & (a["obs_point"] < a["n_points"]), a["obs_point"], a["n_points"]), kind="stable")
    c = dict(a, **{k: np.ascontiguousarray(a[k][order]) for k in ("obs_cam", "obs_point", "obs_xy", "obs_use")})
    three = _run(ctx, c, tc.PARAMS)
    for k in ("point_xyz", "status", "n_good"):
        assert one[k].tobytes() == three[k].tobytes(), k
    assert np.array_equal(three["obs_good"], one["obs_good"][order])


def test_points_start_a_bundle_adjustment(ctx):
    """PnP-registered cameras -> triangulate_tracks -> gh_ba_solve, the outputs unchanged: point_xyz as the start,
    point_free = (status == OK), the observations restricted to obs_good."""
    import torch
    from gslam_amd import ba, estimator
    g = tc.graph(True)
    n_points = len(g["point_xyz"])
    out = estimator.triangulate_tracks(ctx, _dev(g["cam_pose"]), _dev(g["obs_cam"]), _dev(g["obs_point"]), _dev(g["obs_xy"]), n_points,
                                       params=_params(**tc.GRAPH_PARAMS[True]))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = _want(tc.graph_expected(True))
    for k in OUTPUTS:  # the mirror makes the same call
        assert got[k].tobytes() == want[k].tobytes(), k
    keep = got["obs_good"] != 0
    assert keep.sum() == got["n_good"].sum() > 11000
    problem = dict(cam_pose=g["cam_pose"], cam_dof=g["cam_dof"], point_xyz=got["point_xyz"],
                   point_free=(got["status"] == tr.OK).astype(np.uint8), obs_cam=g["obs_cam"][keep], obs_point=g["obs_point"][keep],
                   obs_xy=g["obs_xy"][keep])
    poses, pts, s, st = ba.solve(ctx, problem, ba.default_options())
    assert st == 0
    print("BA from the triangulated start: termination %d after %d iterations, cost %.6e -> %.6e" %
          (s.termination, s.iterations, s.initial_cost, s.final_cost))
    assert s.termination in (1, 2)  # a tolerance, not max_iterations (0) or failure (3)
    assert s.final_cost <= s.initial_cost
