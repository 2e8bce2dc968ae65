"""GPU parity of gh_link_tracks_dev with the plain-Python restatement tests/track_link_restate.py, byte for byte, on the inputs
of tests/track_link_cases.py (tests/test_track_link_cpu.py shows what they reach): the census (and with it the input of
tests/map_wide_cases.py, more than 1024 * 256 nodes), a chain longer than a
workgroup in three pair orders, a hub contended by 256 unions, random windows with wrong rows; the argument contract; then
the call in its place, between exact pair matches and gh_triangulate_tracks_dev.  Output buffers go in dirty (-5 for ints,
7.0 for doubles) and four entries longer than their capacity, so that a write past the end shows too."""
import ctypes as C

import numpy as np
import pytest

import map_wide_cases as wide
import track_link_cases as lc

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS = ("node_point", "obs_cam", "obs_point", "obs_xy", "obs_node", "point_len", "totals")
TAIL = 4


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sizes(N):
    return dict(node_point=N, obs_cam=N, obs_point=N, obs_xy=2 * N, obs_node=N, point_len=N // 2, totals=4)


def _dirty(N):
    import torch
    return {k: torch.full((n + TAIL,), lc.FILL_XY if k == "obs_xy" else lc.FILL_INT, dtype=torch.float64 if k == "obs_xy" else torch.int32,
                          device="cuda") for k, n in _sizes(N).items()}


def _untouched(out, but=()):
    return all((t == (lc.FILL_XY if k == "obs_xy" else lc.FILL_INT)).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_inlier=True):
    d = {k: _dev(c[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1")}
    d["inlier"] = _dev(c["inlier"]) if use_inlier else None
    for k in ("pair_q", "pair_t", "idx1"):  # (an empty tensor has no storage)
        if d[k].numel() == 0:
            d[k] = None
    return d


def _call(ctx_h, d, out, n_frames, cap, npairs, min_views, intrinsics=lc.INTRINSICS):
    from gslam_amd import hip
    fx, fy, cx, cy = intrinsics
    return hip.lib.gh_link_tracks_dev(ctx_h, _ptr(d["kps"]), _ptr(d["counts"]), n_frames, cap, _ptr(d["pair_q"]), _ptr(d["pair_t"]), npairs,
                                      _ptr(d["idx1"]), _ptr(d["inlier"]), C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy),
                                      min_views, *(_ptr(out[k]) for k in OUTPUTS))


def _run(ctx, c, use_inlier=True, min_views=None):
    """gh_link_tracks_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    N = c["n_frames"] * c["cap"]
    out = _dirty(N)
    st = _call(ctx.h, _inputs(c, use_inlier), out, c["n_frames"], c["cap"], len(c["pair_q"]), c["min_views"] if min_views is None else min_views)
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k, n in _sizes(N).items():
        assert (got[k][n:] == (lc.FILL_XY if k == "obs_xy" else lc.FILL_INT)).all(), (c["name"], k, "written past its capacity")
    return {k: got[k][:n].reshape(-1, 2) if k == "obs_xy" else got[k][:n] for k, n in _sizes(N).items()}


def _assert_same(got, e, name):
    N = len(e["node_point"])
    want = lc.as_arrays(e, N)
    assert got["totals"].tolist() == want["totals"].tolist(), (name, got["totals"], want["totals"])
    assert got["node_point"].tolist() == want["node_point"].tolist(), name
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, k)


@pytest.mark.parametrize("min_views", [2, 3])
@pytest.mark.parametrize("use_inlier", [True, False])
def test_census_matches_the_restatement_byte_for_byte(ctx, use_inlier, min_views):
    for c in lc.census():  # per case first: a failure names the case
        _assert_same(_run(ctx, c, use_inlier, min_views), lc.restate(c, use_inlier, min_views), c["name"])
    c = wide.link_case()  # N + 1 > 1024 * 256: the second trip through the loop of link_flags, with verdicts to count in it
    _assert_same(_run(ctx, c, use_inlier, min_views), wide.link_restated(use_inlier, min_views), c["name"])


def test_long_chain_in_any_pair_order_gives_the_same_bytes(ctx):
    first = None
    for order in ("forward", "reversed", "shuffled"):
        c = lc.chain(order, seed=3)
        got = _run(ctx, c)
        _assert_same(got, lc.restate(c), c["name"])
        assert got["totals"].tolist() == [1200, 4, 0, 0] and got["point_len"][:4].tolist() == [300] * 4
        first = first or got
        for k in OUTPUTS:
            assert got[k].tobytes() == first[k].tobytes(), (order, k)


def test_hub_contended_by_256_unions(ctx):
    c = lc.hub()
    got = _run(ctx, c)
    _assert_same(got, lc.restate(c), c["name"])
    assert got["totals"].tolist() == [257, 1, 0, 0] and got["point_len"][0] == 257
    c = lc.hub(conflict=True)
    got = _run(ctx, c)
    _assert_same(got, lc.restate(c), c["name"])
    assert got["totals"].tolist() == [0, 0, 1, 0] and (got["node_point"] == -2).sum() == 258


@pytest.mark.parametrize("use_inlier", [True, False])
def test_random_windows_match_the_restatement_twice(ctx, use_inlier):
    c, with_inlier, without = lc.random_case()
    e = with_inlier if use_inlier else without
    assert e["totals"][2] >= 1 and e["totals"][1] >= 60
    one, two = _run(ctx, c, use_inlier), _run(ctx, c, use_inlier)
    _assert_same(one, e, c["name"])
    for k in OUTPUTS:
        assert one[k].tobytes() == two[k].tobytes(), k


def test_argument_errors_leave_the_outputs_alone(ctx):
    c = lc.census()[0]
    F, cap, P = c["n_frames"], c["cap"], len(c["pair_q"])
    d = _inputs(c)
    out = _dirty(F * cap)
    nan = float("nan")

    def call(ctx_h=ctx.h, sizes=(F, cap, P), min_views=2, intrinsics=lc.INTRINSICS, null=None):
        dd = {k: (None if k == null else t) for k, t in d.items()}
        oo = {k: (None if k == null else t) for k, t in out.items()}
        return _call(ctx_h, dd, oo, sizes[0], sizes[1], sizes[2], min_views, intrinsics)

    assert call(ctx_h=None) == GH_ERR_ARG
    for sizes in ((-1, cap, P), (F, -1, P), (F, cap, -1), (1, 65536, P), (32769, 65535, P), (2**31 - 1, 1, P)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for mv in (1, 0, -3):
        assert call(min_views=mv) == GH_ERR_ARG, mv
    fx, fy, cx, cy = lc.INTRINSICS
    for bad in ((0.0, fy), (-1.0, fy), (nan, fy), (fx, 0.0), (fx, -2.0), (fx, nan)):
        assert call(intrinsics=bad + (cx, cy)) == GH_ERR_ARG, bad
    for k in ("kps", "counts", "pair_q", "pair_t", "idx1") + OUTPUTS:
        assert call(null=k) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: no inlier bytes; no pair arrays when there are no pairs
    assert call(null="inlier") == 0
    ctx.sync()
    assert not _untouched(out, but=("totals",))


def test_degenerate_sizes(ctx):
    import torch
    c = lc.census()[0]
    d = _inputs(c)
    for F, cap in ((0, c["cap"]), (c["n_frames"], 0), (0, 0)):  # N == 0: only totals, zeros
        out = _dirty(c["n_frames"] * c["cap"])
        assert _call(ctx.h, d, out, F, cap, len(c["pair_q"]), 2) == 0
        torch.cuda.synchronize()
        assert _untouched(out, but=("totals",))
        assert out["totals"].cpu().tolist() == [0, 0, 0, 0] + [lc.FILL_INT] * TAIL
    # no pairs: every existing node is SHORT, everything else is padding; the pair arrays may be NULL then
    e = dict(c, pair_q=c["pair_q"][:0], pair_t=c["pair_t"][:0], idx1=c["idx1"][:0], inlier=c["inlier"][:0],
             counts=np.array([8, 5, 0, -2, 11, 1], np.int32), name="no_pairs")
    got = _run(ctx, e, use_inlier=False)
    _assert_same(got, lc.restate(e, False), "no_pairs")
    assert got["totals"].tolist() == [0, 0, 0, 0] and (got["node_point"] == -1).sum() == 8 + 5 + 8 + 1
    assert (got["obs_cam"] == -1).all() and not got["obs_xy"].any() and not got["point_len"].any()


def test_links_exact_matches_into_the_tracks_triangulation_takes(ctx):
    """Exact pair matches of a synthetic graph -> gh_link_tracks_dev -> gh_triangulate_tracks_dev on the padded arrays, no host
    read in between.  The bound on the points: a pixel u = f x + c rounded to float32 moves by at most half an ulp of the largest
    pixel coordinate, the normalised coordinate by that over f, the ray at depth d sideways by d times that (sqrt(2): both
    coordinates), and the intersection of rays that meet at an angle of about baseline / depth by depth / baseline times that;
    with the largest depth and the smallest baseline of the graph this bounds every point."""
    import torch
    from gslam_amd import ba_synth, estimator
    n_cams, n_pts, f, cxy = 8, 200, 500.0, (320.0, 240.0)
    g = ba_synth.make_graph(n_cams, n_pts, 6, seed=2, noise=0.0, outlier_frac=0.0, perturb=False)
    per_cam = [np.flatnonzero(g["obs_cam"] == cam) for cam in range(n_cams)]
    cap = max(len(o) for o in per_cam) + 3
    kps = np.zeros((n_cams, cap, 7), np.float32)
    row_of = -np.ones((n_cams, n_pts), np.int64)
    for cam, obs in enumerate(per_cam):
        kps[cam, :len(obs), 0] = (f * g["obs_xy"][obs, 0] + cxy[0]).astype(np.float32)
        kps[cam, :len(obs), 1] = (f * g["obs_xy"][obs, 1] + cxy[1]).astype(np.float32)
        row_of[cam, g["obs_point"][obs]] = np.arange(len(obs))
    pairs = [(q, t) for q in range(n_cams) for t in range(q + 1, n_cams)]
    assert len(pairs) == 28
    idx1 = np.full((len(pairs), cap), -1, np.int32)
    for k, (q, t) in enumerate(pairs):
        both = np.flatnonzero((row_of[q] >= 0) & (row_of[t] >= 0))
        idx1[k, row_of[q, both]] = row_of[t, both]
    counts = np.array([len(o) for o in per_cam], np.int32)
    N = n_cams * cap
    poses = _dev(g["cam_pose_gt"])
    link = estimator.link_tracks(ctx, _dev(kps), _dev(counts), _dev(np.array([p[0] for p in pairs], np.int32)),
                                 _dev(np.array([p[1] for p in pairs], np.int32)), _dev(idx1), None, (f, f) + cxy)
    padded = estimator.triangulate_tracks(ctx, poses, link["obs_cam"], link["obs_point"], link["obs_xy"], N // 2)
    torch.cuda.synchronize()

    n_obs, n_points = link["totals"].cpu().tolist()[:2]
    assert n_points == n_pts and n_obs == len(g["obs_cam"]) and link["totals"].cpu().tolist()[2:] == [0, 0]
    node, point = link["obs_node"].cpu().numpy()[:n_obs], link["obs_point"].cpu().numpy()[:n_obs]
    got_sets = {}
    for n, p in zip(node.tolist(), point.tolist()):
        got_sets.setdefault(p, set()).add(n)
    true_sets = {}
    for cam, p in zip(g["obs_cam"].tolist(), g["obs_point"].tolist()):
        true_sets.setdefault(p, set()).add(cam * cap + int(row_of[cam, p]))
    assert sorted(map(sorted, got_sets.values())) == sorted(map(sorted, true_sets.values()))  # the ground-truth partition
    gt_of = np.array([g["obs_point"][per_cam[min(s) // cap][min(s) % cap]] for _, s in sorted(got_sets.items())])

    cut = estimator.triangulate_tracks(ctx, poses, link["obs_cam"][:n_obs].contiguous(), link["obs_point"][:n_obs].contiguous(),
                                       link["obs_xy"][:n_obs].contiguous(), n_points)
    torch.cuda.synchronize()
    status, xyz = padded["status"].cpu().numpy(), padded["point_xyz"].cpu().numpy()
    assert status[:n_points].tobytes() == cut["status"].cpu().numpy().tobytes()
    assert xyz[:n_points].tobytes() == cut["point_xyz"].cpu().numpy().tobytes()
    assert padded["n_good"].cpu().numpy()[:n_points].tobytes() == cut["n_good"].cpu().numpy().tobytes()
    assert padded["obs_good"].cpu().numpy()[:n_obs].tobytes() == cut["obs_good"].cpu().numpy().tobytes()
    assert (status[n_points:] == estimator.TRACK_TOO_FEW).all() and not padded["obs_good"].cpu().numpy()[n_obs:].any()

    ok = status[:n_points] == estimator.TRACK_OK
    half_ulp = float(np.spacing(np.float32(np.abs(kps[..., :2]).max()))) / 2
    pos = g["cam_pose_gt"][:, 4:]
    depth = np.linalg.norm(g["point_xyz_gt"][g["obs_point"]] - pos[g["obs_cam"]], axis=1).max()
    baseline = min(np.linalg.norm(pos[a] - pos[b]) for a, b in pairs)
    bound = np.sqrt(2.0) * half_ulp / f * depth * (depth / baseline)
    err = np.linalg.norm(xyz[:n_points] - g["point_xyz_gt"][gt_of], axis=1)
    print("OK points %d of %d, largest error %.3e, bound %.3e" % (ok.sum(), n_points, err[ok].max(), bound))
    assert ok.all() and err[ok].max() <= bound
