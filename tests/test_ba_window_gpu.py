"""GPU parity of gh_ba_window_dev with the plain-Python restatement tests/ba_window_restate.py, byte for byte, on the inputs of
tests/ba_window_cases.py (tests/test_ba_window_cpu.py shows what they reach): the census, the soups at the block boundaries of
every launch, the hub in two orders and the trajectory at two thresholds in three orders; the empty forms and the argument
contract; gh_ba_window_scatter_dev; then the call in its place: window -> gh_ba_solve -> scatter on the trajectory, and at the
end of link -> triangulate -> localize -> extend -> triangulate the new points, without a read-back before it.  Every output
buffer goes in with every byte 0xA5 and 16 bytes longer than its capacity, so that an entry left out and a write past the end
both show; every input carries 16 bytes of tail as well, so that an array of no entries still has an address."""
import ctypes as C

import numpy as np
import pytest

import ba_window_cases as wc
import ba_window_restate as rs

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS = wc.OUTPUTS
INPUTS = ("cam_pose", "point_xyz", "obs_cam", "obs_point", "obs_xy", "obs_use", "point_use", "cam_seed", "cam_hold")
TAIL = 16
FILL = 0xA5


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    """The bytes of `a` on the device, followed by TAIL zero bytes."""
    import torch
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return torch.from_numpy(np.concatenate([raw, np.zeros(TAIL, np.uint8)])).cuda()


def _counts(c):
    return c["n_cams"], c["n_points"], len(c["obs_cam"])


def _dirty(n_cams, n_points, n_obs):
    import torch
    return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in wc.sizes(n_cams, n_points, n_obs).items()}


def _untouched(out):
    return all((t == FILL).all().item() for t in out.values())


def _inputs(c, use_obs_use=True, use_point_use=True, use_hold=True):
    d = {k: _dev(c[k]) for k in INPUTS}
    for k, use in (("obs_use", use_obs_use), ("point_use", use_point_use), ("cam_hold", use_hold)):
        if not use:
            d[k] = None
    return d


def _call(ctx_h, d, out, counts, min_shared, min_point_obs, params=True):
    from gslam_amd import hip
    par = hip.BaWindowParams(min_shared, min_point_obs)
    return hip.lib.gh_ba_window_dev(ctx_h, *counts, *(_ptr(d[k]) for k in INPUTS), C.byref(par) if params else None,
                                    *(_ptr(out[k]) for k in OUTPUTS))


def _host(out, counts):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k, n in wc.sizes(*counts).items():
        raw = out[k].cpu().numpy()
        assert (raw[n:] == FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(wc.DTYPE[k])
    return got


def _run(ctx, c, use_obs_use=True, use_point_use=True, use_hold=True, min_shared=None, min_point_obs=None, twice=False):
    """gh_ba_window_dev on dirty output buffers -> dict of flat host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    counts = _counts(c)
    d = _inputs(c, use_obs_use, use_point_use, use_hold)
    ms = c["min_shared"] if min_shared is None else min_shared
    mp = c["min_point_obs"] if min_point_obs is None else min_point_obs
    results = []
    for _ in range(2 if twice else 1):
        out = _dirty(*counts)
        st = _call(ctx.h, d, out, counts, ms, mp)
        assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
        torch.cuda.synchronize()
        results.append(_host(out, counts))
    if twice:
        for k in OUTPUTS:
            assert results[0][k].tobytes() == results[1][k].tobytes(), (c["name"], k, "the second call differs")
    return results[0]


def _assert_same(got, want, name):
    assert got["totals"].tolist() == want["totals"].tolist(), (name, got["totals"], want["totals"])
    for k in ("cam_class", "cam_shared", "cam_slot", "win_cam", "win_cam_dof"):
        assert got[k].tolist() == want[k].tolist(), (name, k)
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, k)


# obs_use, point_use, cam_hold given?  Every optional input also as NULL, alone and together
VARIANTS = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]


@pytest.mark.parametrize("min_shared,min_point_obs", [(3, 2), (0, 2), (1, 1), (4, 3)])
@pytest.mark.parametrize("use_obs_use,use_point_use,use_hold", VARIANTS)
def test_census_matches_the_restatement_byte_for_byte(ctx, use_obs_use, use_point_use, use_hold, min_shared, min_point_obs):
    c = wc.census()
    got = _run(ctx, c, use_obs_use, use_point_use, use_hold, min_shared, min_point_obs, twice=True)
    _assert_same(got, wc.as_arrays(wc.restate(c, use_obs_use, use_point_use, use_hold, min_shared, min_point_obs)), c["name"])
    if (use_obs_use, use_point_use, use_hold, min_shared, min_point_obs) == (True, True, True, 3, 2):
        assert got["totals"].tolist() == [6, 4, 2, 2, 6, 18, 2, 24] and got["cam_class"].tolist() == [2, 0, 2, 1, 1, 0, 1, 1]


@pytest.mark.parametrize("which", range(6))
def test_block_boundaries(ctx, which):
    c = wc.boundaries()[which]
    assert _counts(c) == [(40, 100, 512), (40, 100, 513), (256, 90, 1500), (257, 90, 1500), (40, 512, 1500), (40, 513, 1500)][which]
    for v in (VARIANTS[0], VARIANTS[-1]):
        _assert_same(_run(ctx, c, *v, twice=True), wc.as_arrays(wc.restate(c, *v)), c["name"])
    _assert_same(_run(ctx, c, min_shared=0, min_point_obs=1), wc.as_arrays(wc.restate(c, min_shared=0, min_point_obs=1)), c["name"])


def test_hub_counts_are_exact_in_both_orders(ctx):
    """257 observations of one point and 3001 of one camera: more than a workgroup's lanes on one word, as one run of equal keys
    (frame-major for the camera, track-major for the point) and scattered."""
    c, want = wc.restated("hub")
    got = _run(ctx, c, twice=True)
    _assert_same(got, want, c["name"])
    assert got["totals"].tolist() == [257, 185, 72, 2, 3001, 6257, 1, 6257]
    assert got["cam_shared"].tolist() == [12] + [13] * 184 + [12] * 71 + [3001]
    for d in (wc.hub("track_major"), wc.reorder(c, "shuffled", seed=9)[0]):
        other = _run(ctx, d)
        _assert_same(other, wc.as_arrays(wc.restate(d)), d["name"])
        for k in OUTPUTS:
            if k not in wc.OBS_OUTPUTS:
                assert other[k].tobytes() == got[k].tobytes(), (d["name"], k)
    for v in VARIANTS[1:]:
        _assert_same(_run(ctx, c, *v), wc.as_arrays(wc.restate(c, *v)), c["name"])


@pytest.mark.parametrize("min_shared", [15, 1])
def test_trajectory_in_three_orders_gives_the_same_window(ctx, min_shared):
    c, want = wc.restated("trajectory_%d" % min_shared)
    first = None
    for order in ("forward", "reversed", "shuffled"):
        d, perm = wc.reorder(c, order, seed=5)
        got = _run(ctx, d, twice=(order == "forward"))
        if order == "forward":
            _assert_same(got, want, d["name"])
            t = got["totals"].tolist()
            assert (t[1], t[2], t[4], t[5]) == wc.TRAJECTORY_FIGURES[min_shared] and got["cam_shared"][50] == 2
        else:
            _assert_same(got, wc.as_arrays(wc.restate(d)), d["name"])
        view = ([got[k].tobytes() for k in OUTPUTS if k not in wc.OBS_OUTPUTS], wc.in_source_order(got, perm))
        first = first or view
        assert view == first, order
    _assert_same(_run(ctx, c, False, False, False), wc.as_arrays(wc.restate(c, False, False, False)), c["name"])


def _cut(c, n_cams=None, n_points=None, n_obs=None):
    """The case with a capacity cut down: the arrays that capacity sizes are cut with it."""
    d = dict(c, name="%s_cut_%s_%s_%s" % (c["name"], n_cams, n_points, n_obs))
    if n_cams is not None:
        d.update(n_cams=n_cams, cam_pose=c["cam_pose"][:n_cams], cam_seed=c["cam_seed"][:n_cams], cam_hold=c["cam_hold"][:n_cams])
    if n_points is not None:
        d.update(n_points=n_points, point_xyz=c["point_xyz"][:n_points], point_use=c["point_use"][:n_points])
    if n_obs is not None:
        d.update(obs_cam=c["obs_cam"][:n_obs], obs_point=c["obs_point"][:n_obs], obs_xy=c["obs_xy"][:n_obs], obs_use=c["obs_use"][:n_obs])
    return d


def test_empty_forms(ctx):
    c = wc.census()
    nc, npts, no = _counts(c)
    # no seed: an empty window; the usable observations are still counted
    d = dict(c, cam_seed=np.zeros(nc, np.uint8), name="no_seed")
    got = _run(ctx, d, twice=True)
    _assert_same(got, wc.as_arrays(wc.restate(d)), d["name"])
    assert got["totals"].tolist() == [0] * 7 + [24] and not got["cam_class"].any() and not got["cam_shared"].any()
    assert (got["cam_slot"] == -1).all() and (got["point_slot"] == -1).all() and (got["win_obs_src"] == -1).all()
    assert (got["win_cam"] == -1).all() and not got["win_cam_pose"].view(np.uint8).any() and not got["win_obs_xy"].view(np.uint8).any()
    # n_obs == 0
    d = _cut(c, n_obs=0)
    got = _run(ctx, d)
    _assert_same(got, wc.as_arrays(wc.restate(d)), d["name"])
    assert got["totals"].tolist() == [0] * 8 and not got["cam_class"].any() and (got["win_point"] == -1).all()
    # n_points == 0: no observation is usable
    d = _cut(c, n_points=0)
    got = _run(ctx, d)
    _assert_same(got, wc.as_arrays(wc.restate(d)), d["name"])
    assert got["totals"].tolist() == [0] * 8 and (got["win_obs_cam"] == -1).all() and (got["win_cam"] == -1).all()
    # n_cams == 0: the totals are zeros, the point and observation outputs are padding
    d = _cut(c, n_cams=0)
    got = _run(ctx, d)
    _assert_same(got, wc.as_arrays(wc.restate(d)), d["name"])
    assert got["totals"].tolist() == [0] * 8 and (got["point_slot"] == -1).all() and (got["win_point"] == -1).all()
    assert (got["win_obs_src"] == -1).all() and not got["win_point_xyz"].view(np.uint8).any()
    # nothing at all: the totals only
    d = _cut(c, 0, 0, 0)
    assert _run(ctx, d)["totals"].tolist() == [0] * 8
    # cameras and points, no observations and the reverse, on one more soup
    s = wc.boundaries()[0]
    for d in (_cut(s, n_obs=1), _cut(s, n_cams=1), _cut(s, n_points=1)):
        _assert_same(_run(ctx, d), wc.as_arrays(wc.restate(d)), d["name"])


def test_argument_errors_leave_the_outputs_alone(ctx):
    c = wc.census()
    counts = _counts(c)
    d = _inputs(c)
    out = _dirty(*counts)

    def call(ctx_h=ctx.h, counts=counts, min_shared=3, min_point_obs=2, null=(), params=True):
        dd = {k: (None if k in null else t) for k, t in d.items()}
        oo = {k: (None if k in null else t) for k, t in out.items()}
        return _call(ctx_h, dd, oo, counts, min_shared, min_point_obs, params)

    assert call(ctx_h=None) == GH_ERR_ARG
    assert call(params=False) == GH_ERR_ARG
    for bad in ((-1, 12, 34), (8, -1, 34), (8, 12, -1), (-2**31, 12, 34)):
        assert call(counts=bad) == GH_ERR_ARG, bad
    for ms in (-1, -2**31):
        assert call(min_shared=ms) == GH_ERR_ARG, ms
    for mp in (0, -1, -2**31):
        assert call(min_point_obs=mp) == GH_ERR_ARG, mp
    for k in ("cam_seed", "cam_pose", "point_xyz", "obs_cam", "obs_point", "obs_xy") + OUTPUTS:
        assert call(null=(k,)) == GH_ERR_ARG, k
    for k in ("cam_seed",) + OUTPUTS:  # (these even when the count that sizes them is zero)
        assert call(counts=(0, 0, 0), null=(k,)) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: an array of no entries may be NULL, and so may the three optional inputs
    assert call(counts=(0, 12, 34), null=("cam_pose",)) == 0
    assert call(counts=(8, 0, 34), null=("point_xyz",)) == 0
    assert call(counts=(8, 12, 0), null=("obs_cam", "obs_point", "obs_xy")) == 0
    for null in (("obs_use",), ("point_use",), ("cam_hold",), ("obs_use", "point_use", "cam_hold")):
        assert call(null=null) == 0, null
    ctx.sync()
    assert not any((t[:-TAIL] == FILL).all().item() for t in out.values()) and all((t[-TAIL:] == FILL).all().item() for t in out.values())


def _scatter(ctx_h, a, counts):
    from gslam_amd import hip
    n_win_cams, n_win_points, n_cams, n_points = counts
    return hip.lib.gh_ba_window_scatter_dev(ctx_h, _ptr(a["win_cam"]), _ptr(a["win_cam_dof"]), n_win_cams, _ptr(a["cam_pose_win"]),
                                            _ptr(a["win_point"]), n_win_points, _ptr(a["point_xyz_win"]), _ptr(a["cam_pose"]), n_cams,
                                            _ptr(a["point_xyz"]), n_points)


def test_scatter_lands_in_exactly_the_rows_named(ctx):
    import torch
    n_cams, n_points, nwc, nwp = 300, 700, 260, 520  # more than one workgroup of each
    rng = np.random.default_rng(3)
    win_cam = rng.permutation(n_cams)[:nwc].astype(np.int32)
    win_cam_dof = rng.choice(np.array([0, 0, 63, 63, 63, 1, 64], np.int32), nwc)  # FIXED and held: 0; anything else moves
    win_cam[[5, 77, 259]] = [-1, n_cams, 2**31 - 1]                               # out of range with a dof: dropped
    win_cam_dof[[5, 77, 259]] = 63
    win_point = rng.permutation(n_points)[:nwp].astype(np.int32)
    win_point[[0, 300, 519]] = [-7, n_points, -2**31]
    pose_win, xyz_win = rng.standard_normal((nwc, 7)), rng.standard_normal((nwp, 3))
    pose_win[3, 2], xyz_win[4, 1] = np.nan, -0.0                                  # bits, not values
    pose, xyz = rng.standard_normal((n_cams, 7)), rng.standard_normal((n_points, 3))
    host = dict(win_cam=win_cam, win_cam_dof=win_cam_dof, cam_pose_win=pose_win, win_point=win_point, point_xyz_win=xyz_win, cam_pose=pose,
                point_xyz=xyz)
    # the lists are longer than the counts passed: the entries past them must not land
    n_used_cams, n_used_points = nwc - 3, nwp - 2
    want_pose, want_xyz = pose.copy(), xyz.copy()
    for i in range(n_used_cams):
        if win_cam_dof[i] != 0 and 0 <= win_cam[i] < n_cams:
            want_pose[win_cam[i]] = pose_win[i]
    for j in range(n_used_points):
        if 0 <= win_point[j] < n_points:
            want_xyz[win_point[j]] = xyz_win[j]
    r_pose, r_xyz = rs.scatter(win_cam.tolist(), win_cam_dof.tolist(), n_used_cams, pose_win.tolist(), win_point.tolist(), n_used_points,
                               xyz_win.tolist(), pose.tolist(), xyz.tolist())
    assert np.array(r_pose).tobytes() == want_pose.tobytes() and np.array(r_xyz).tobytes() == want_xyz.tobytes()
    a = {k: _dev(v) for k, v in host.items()}
    assert _scatter(ctx.h, a, (n_used_cams, n_used_points, n_cams, n_points)) == 0
    torch.cuda.synchronize()
    got_pose, got_xyz = a["cam_pose"].cpu().numpy(), a["point_xyz"].cpu().numpy()
    assert got_pose[:-TAIL].tobytes() == want_pose.tobytes() and not got_pose[-TAIL:].any()
    assert got_xyz[:-TAIL].tobytes() == want_xyz.tobytes() and not got_xyz[-TAIL:].any()
    moved = np.flatnonzero((want_pose.view(np.uint64) != pose.view(np.uint64)).any(1))
    assert 100 < len(moved) < n_used_cams and len(np.flatnonzero((want_xyz.view(np.uint64) != xyz.view(np.uint64)).any(1))) == n_used_points - 2
    # errors and empty calls change nothing
    before = (a["cam_pose"].clone(), a["point_xyz"].clone())
    assert _scatter(None, a, (1, 1, n_cams, n_points)) == GH_ERR_ARG
    for bad in ((-1, 1, n_cams, n_points), (1, -1, n_cams, n_points), (1, 1, -1, n_points), (1, 1, n_cams, -1)):
        assert _scatter(ctx.h, a, bad) == GH_ERR_ARG, bad
    for k in ("win_cam", "win_cam_dof", "cam_pose_win", "win_point", "point_xyz_win", "cam_pose", "point_xyz"):
        assert _scatter(ctx.h, dict(a, **{k: None}), (1, 1, n_cams, n_points)) == GH_ERR_ARG, k
    assert _scatter(ctx.h, a, (0, 0, n_cams, n_points)) == 0 and _scatter(ctx.h, a, (nwc, nwp, 0, 0)) == 0
    torch.cuda.synchronize()
    assert torch.equal(before[0], a["cam_pose"]) and torch.equal(before[1], a["point_xyz"])


def _problem_of(e, c):
    """The gh_ba_problem the restatement builds from the host arrays."""
    t = e["totals"]
    cut = lambda k, n: np.array(e[k][:n], wc.DTYPE[k])
    return {"cam_pose": cut("win_cam_pose", t[0]).reshape(-1, 7), "cam_dof": cut("win_cam_dof", t[0]),
            "point_xyz": cut("win_point_xyz", t[4]).reshape(-1, 3), "obs_cam": cut("win_obs_cam", t[5]), "obs_point": cut("win_obs_point", t[5]),
            "obs_xy": cut("win_obs_xy", t[5]).reshape(-1, 2), "win_cam": cut("win_cam", t[0]), "win_point": cut("win_point", t[4])}


PROBLEM_KEYS = ("cam_pose", "cam_dof", "point_xyz", "obs_cam", "obs_point", "obs_xy", "win_cam", "win_point")


def _trace(s):
    n = s.trace_len
    return (s.iterations, s.accepted, s.termination, s.initial_cost, s.final_cost, n, list(s.trace_cost[:n]), list(s.trace_radius[:n]),
            list(s.trace_accepted[:n]))


def test_window_solve_scatter_end_to_end(ctx):
    """The perturbed trajectory: window at min_shared 15 -> window_problem -> ba.solve -> window_scatter.  The termination reason
    is printed, not asserted: nobody has run this window through the solver before."""
    import torch
    from gslam_amd import ba
    c = wc.trajectory(15, perturb=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cam_pose, point_xyz = dev(c["cam_pose"]), dev(c["point_xyz"])
    win = ba.window(ctx, cam_pose, point_xyz, dev(c["obs_cam"]), dev(c["obs_point"]), dev(c["obs_xy"]), dev(c["cam_seed"]),
                    obs_use=dev(c["obs_use"]), point_use=dev(c["point_use"]), cam_hold=dev(c["cam_hold"]), min_shared=15)
    prob = ba.window_problem(win)
    e = wc.restate(c)
    want = _problem_of(e, c)
    assert prob["totals"] == e["totals"] and (prob["totals"][1], prob["totals"][2], prob["totals"][4], prob["totals"][5]) == wc.TRAJECTORY_FIGURES[15]
    for k in PROBLEM_KEYS:
        assert prob[k].dtype == want[k].dtype and prob[k].shape == want[k].shape and prob[k].tobytes() == want[k].tobytes(), k
    opts = ba.default_options(max_iterations=30)
    poses, points, s, st = ba.solve(ctx, prob, opts)
    poses2, points2, s2, st2 = ba.solve(ctx, want, ba.default_options(max_iterations=30))
    assert st == st2 and poses.tobytes() == poses2.tobytes() and points.tobytes() == points2.tobytes() and _trace(s) == _trace(s2)
    print("window of %d cameras (%d LOCAL), %d points, %d observations: status %d, termination %d after %d iterations, cost %.6e -> %.6e" %
          (prob["totals"][0], prob["totals"][1], prob["totals"][4], prob["totals"][5], st, s.termination, s.iterations, s.initial_cost,
           s.final_cost))
    assert s.final_cost <= s.initial_cost
    ba.window_scatter(ctx, win, poses, points, cam_pose, point_xyz)
    torch.cuda.synchronize()
    want_pose, want_xyz = c["cam_pose"].copy(), c["point_xyz"].copy()
    local = np.flatnonzero(prob["cam_dof"] != 0)
    assert len(local) == 9 and (np.array(e["cam_class"])[prob["win_cam"][local]] == rs.WIN_LOCAL).all()
    want_pose[prob["win_cam"][local]] = poses[local]
    want_xyz[prob["win_point"]] = points
    assert cam_pose.cpu().numpy().tobytes() == want_pose.tobytes() and point_xyz.cpu().numpy().tobytes() == want_xyz.tobytes()
    fixed = prob["win_cam"][prob["cam_dof"] == 0]
    assert len(fixed) == 8 and want_pose[fixed].tobytes() == c["cam_pose"][fixed].tobytes()
    assert (want_pose[prob["win_cam"][local]] != c["cam_pose"][prob["win_cam"][local]]).any(1).all()   # the solve moved every LOCAL camera


def test_the_loop_closes_with_a_window_of_the_new_frames(ctx):
    """track_extend_cases.scene(late_points=True): link -> triangulate -> localize -> extend -> triangulate the new points, as in
    tests/test_track_extend_gpu.py, then the window of the three new frames on the arrays as they lie on the device: obs_use is
    obs_good merged over the two triangulations (an observation the localisation adopted counts with its row_inlier byte: the
    PnP judged it), point_use is status == OK merged the same way, both with torch on the device.  Nothing is read back before
    window_problem."""
    import torch
    import localize_cases as loc
    import track_extend_cases as ec
    from gslam_amd import ba, estimator
    s = ec.scene(True)
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    n_map_pts = N // 2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kps, counts = dev(s["kps"]), dev(s["counts"])
    link = estimator.link_tracks(ctx, kps, counts, dev(s["map_q"]), dev(s["map_t"]), dev(s["map_idx1"]), None, s["intrinsics"])
    tri = estimator.triangulate_tracks(ctx, dev(s["poses"]), link["obs_cam"], link["obs_point"], link["obs_xy"], n_map_pts)
    locz = estimator.localize_pairs(ctx, kps, counts, dev(s["new_q"]), dev(s["new_t"]), dev(s["new_idx1"]), None, link["node_point"],
                                    tri["point_xyz"], tri["status"], s["intrinsics"], ransac_threshold=loc.SCENE_RANSAC_THRESHOLD,
                                    seed=loc.SCENE_SEED, inlier_threshold=loc.SCENE_INLIER_THRESHOLD)
    ext = estimator.extend_tracks(ctx, kps, counts, dev(s["ext_q"]), dev(s["ext_t"]), dev(s["ext_idx1"]), None, link["node_point"], n_map_pts,
                                  locz["row_point"], locz["row_inlier"], s["intrinsics"])
    poses = dev(s["poses"])
    poses[loc.SCENE_MAP:] = locz["poses"][loc.SCENE_MAP:]
    PC = n_map_pts + N // 2
    xyz = torch.zeros((PC, 3), dtype=torch.float64, device="cuda")
    xyz[:n_map_pts] = tri["point_xyz"]
    tri2 = estimator.triangulate_tracks(ctx, poses, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], PC, point_select=ext["point_new"],
                                        point_xyz=xyz)
    # the merges, on the device
    point_use = (tri2["status"] == estimator.TRACK_OK)
    point_use[:n_map_pts] = tri["status"] == estimator.TRACK_OK
    point_use = point_use.to(torch.uint8).contiguous()
    good_node = torch.zeros(N + 1, dtype=torch.uint8, device="cuda")       # obs_good of the first triangulation, by keypoint row
    first_node = link["obs_node"].long()
    good_node[torch.where(first_node >= 0, first_node, torch.full_like(first_node, N))] = tri["obs_good"]
    good_node[N] = 0
    node = ext["obs_node"].long()
    row = node.clamp(min=0)
    adopted = (link["node_point"][row] < 0) & (ext["obs_point"] >= 0) & (ext["obs_point"] < n_map_pts) & (locz["row_inlier"].reshape(-1)[row] != 0)
    obs_use = (((tri2["obs_good"] != 0) | (good_node[row] != 0) | adopted) & (node >= 0)).to(torch.uint8).contiguous()
    cam_seed = torch.zeros(F, dtype=torch.uint8, device="cuda")
    cam_seed[loc.SCENE_MAP:] = 1
    cam_hold = torch.zeros(F, dtype=torch.uint8, device="cuda")
    cam_hold[0] = 1
    point_xyz = tri2["point_xyz"]
    win = ba.window(ctx, poses, point_xyz, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], cam_seed, obs_use=obs_use, point_use=point_use,
                    cam_hold=cam_hold)
    prob = ba.window_problem(win)   # the first read-back

    host = lambda t: t.cpu().numpy()
    h_use, h_point_use = host(obs_use), host(point_use)
    c = dict(name="scene_window", n_cams=F, n_points=PC, cam_pose=host(poses), point_xyz=host(point_xyz), obs_cam=host(ext["obs_cam"]),
             obs_point=host(ext["obs_point"]), obs_xy=host(ext["obs_xy"]), obs_use=h_use, point_use=h_point_use, cam_seed=host(cam_seed),
             cam_hold=host(cam_hold), min_shared=15, min_point_obs=2)
    want = wc.as_arrays(wc.restate(c))
    for k in OUTPUTS:
        got = host(win[k]).reshape(-1)
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k
    t = prob["totals"]
    ext_totals = host(ext["totals"]).tolist()
    print("map: %d frames, %d observations, %d points (%d OK), %d good observations; window: cameras %d (LOCAL %d, FIXED %d, held %d), "
          "points %d, observations %d, seeds %d, usable %d" % (F, ext_totals[0], ext_totals[1], int(h_point_use.sum()), int(h_use.sum()), *t))
    assert t[6] == F - loc.SCENE_MAP and t[1] >= t[6] and t[4] > 0 and t[5] >= 2 * t[4] and t[7] <= int((h_use != 0).sum())
    # every window index is in range
    assert len(prob["cam_pose"]) == t[0] and len(prob["point_xyz"]) == t[4] and len(prob["obs_cam"]) == t[5]
    assert ((prob["obs_cam"] >= 0) & (prob["obs_cam"] < t[0])).all() and ((prob["obs_point"] >= 0) & (prob["obs_point"] < t[4])).all()
    assert ((prob["win_cam"] >= 0) & (prob["win_cam"] < F)).all() and ((prob["win_point"] >= 0) & (prob["win_point"] < PC)).all()
    src = prob["win_obs_src"]
    assert ((src >= 0) & (src < ext_totals[0])).all() and (np.diff(src) > 0).all()
    # no window observation is one the map does not vouch for
    assert (h_use[src] != 0).all() and (h_point_use[c["obs_point"][src]] != 0).all()
    assert (prob["win_cam"][prob["obs_cam"]] == c["obs_cam"][src]).all() and (prob["win_point"][prob["obs_point"]] == c["obs_point"][src]).all()
    assert prob["cam_dof"][prob["win_cam"] == 0].tolist() in ([], [0])   # frame 0 is held wherever it takes part
    poses_out, points_out, summary, st = ba.solve(ctx, prob, ba.default_options(max_iterations=10))
    print("gh_ba_solve on the window: status %d, termination %d after %d iterations, cost %.6e -> %.6e" %
          (st, summary.termination, summary.iterations, summary.initial_cost, summary.final_cost))
    assert st == 0
