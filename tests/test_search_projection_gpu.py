"""GPU parity of gh_search_projection_dev with the plain-Python restatement tests/search_projection_restate.py, byte for byte, on
the inputs of tests/search_projection_cases.py (tests/test_search_projection_cpu.py shows what they reach) with each optional
input given and NULL; two runs; in place against disjoint; the argument contract; the degenerate sizes; then the call in its
place on localize_cases.scene(): link -> triangulate -> describe -> localize -> search in place on localize's claims and poses
-> extend, without a read-back in between.  Every output buffer goes in with every byte 0xA5 and 16 bytes longer than its
capacity, so that an entry left out and a write past the end both show."""
import collections
import ctypes as C

import numpy as np
import pytest

import localize_cases as loc
import search_projection_cases as sc
import search_projection_restate as sr
import track_extend_cases as ec
from test_point_describe_gpu import _scene_desc

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS, DTYPE = sc.OUTPUTS, sc.DTYPE
TAIL = 16
FILL = loc.FILL
CASES = {c["name"]: c for c in sc.cases()}
INPUTS = ("kps", "desc", "counts", "poses", "frame_search", "node_point", "row_point", "row_inlier", "xyz", "status", "select", "views",
          "point_desc", "normal", "dist")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(n_frames, cap):
    N = n_frames * cap
    return dict(row_point=4 * N, row_inlier=N, row_dist=2 * N, frame_totals=40 * n_frames, totals=48)


def _dirty(n_frames, cap):
    import torch
    return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in _bytes(n_frames, cap).items()}


def _untouched(out, but=()):
    return all((t == FILL).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_map=True, use_claims=True, use_status=True, use_select=True):
    d = {k: _dev(c[k]) for k in INPUTS}
    for k, use in (("node_point", use_map), ("row_point", use_claims), ("row_inlier", use_claims), ("status", use_status),
                   ("select", use_select)):
        if not use:
            d[k] = None
    return d


def _params(prm):
    from gslam_amd import hip
    return hip.SearchParams(**prm)


def _call(ctx_h, d, out, sizes, params, intrinsics=sc.INTRINSICS, size=sc.SIZE):
    from gslam_amd import hip
    F, cap, P = sizes
    return hip.lib.gh_search_projection_dev(
        ctx_h, _ptr(d["kps"]), _ptr(d["desc"]), _ptr(d["counts"]), F, cap, _ptr(d["poses"]), _ptr(d["frame_search"]),
        _ptr(d["node_point"]), _ptr(d["row_point"]), _ptr(d["row_inlier"]), P, _ptr(d["xyz"]), _ptr(d["status"]), _ptr(d["select"]),
        _ptr(d["views"]), _ptr(d["point_desc"]), _ptr(d["normal"]), _ptr(d["dist"]), *(C.c_double(v) for v in intrinsics),
        int(size[0]), int(size[1]), C.byref(params) if params is not None else None, *(_ptr(out[k]) for k in OUTPUTS))


def _sizes(c):
    return c["n_frames"], c["cap"], c["n_points"]


def _host(out, n_frames, cap):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k, n in _bytes(n_frames, cap).items():
        raw = out[k].cpu().numpy()
        assert (raw[n:] == FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(DTYPE[k])
    got["frame_totals"] = got["frame_totals"].reshape(n_frames, 10)
    return got


def _run(ctx, c, *variant):
    """gh_search_projection_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    out = _dirty(c["n_frames"], c["cap"])
    st = _call(ctx.h, _inputs(c, *variant), out, _sizes(c), _params(c["params"]), c["intrinsics"], c["size"])
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return _host(out, c["n_frames"], c["cap"])


def _assert_same(got, want, name, note=()):
    assert got["totals"].tolist() == want["totals"].tolist(), (name, note, got["totals"], want["totals"])
    assert got["frame_totals"].tolist() == want["frame_totals"].tolist(), (name, note)
    for k in ("row_point", "row_inlier", "row_dist"):
        if got[k].tobytes() != want[k].tobytes():
            raise AssertionError((name, note, k, "nodes", np.flatnonzero(got[k] != want[k])[:10].tolist()))


@pytest.mark.parametrize("name", list(CASES))
def test_cases_match_the_restatement_byte_for_byte(ctx, name):
    c = CASES[name]
    for v in sc.VARIANTS:
        want = sc.as_arrays(sc.restate(c, *v), c["n_frames"])
        _assert_same(_run(ctx, c, *v), want, name, v)


def test_two_runs_give_equal_bytes(ctx):
    for c in (sc.soup(), sc.windows()):
        a, b = _run(ctx, c), _run(ctx, c)
        assert all(a[k].tobytes() == b[k].tobytes() for k in OUTPUTS), c["name"]


def test_in_place_equals_disjoint(ctx):
    import torch
    for c in (sc.soup(), sc.windows(), sc.edges()):
        want = _run(ctx, c)
        d = _inputs(c)
        out = _dirty(c["n_frames"], c["cap"])
        out["row_point"], out["row_inlier"] = d["row_point"].view(torch.uint8), d["row_inlier"]
        assert _call(ctx.h, d, out, _sizes(c), _params(c["params"]), c["intrinsics"], c["size"]) == 0
        torch.cuda.synchronize()
        assert d["row_point"].cpu().numpy().tobytes() == want["row_point"].tobytes(), c["name"]
        assert d["row_inlier"].cpu().numpy().tobytes() == want["row_inlier"].tobytes(), c["name"]
        got = {k: out[k].cpu().numpy()[:-TAIL].view(DTYPE[k]) for k in ("row_dist", "frame_totals", "totals")}
        assert all(got[k].tobytes() == want[k].tobytes() for k in got), c["name"]


def test_argument_errors_leave_the_outputs_alone(ctx):
    from gslam_amd import hip
    c = sc.soup()
    F, cap, P = _sizes(c)
    d = _inputs(c)
    out = _dirty(F, cap)
    nan, inf = float("nan"), float("inf")

    def call(ctx_h=ctx.h, sizes=(F, cap, P), params=(), null=(), shift=(), intrinsics=sc.INTRINSICS, size=sc.SIZE):
        dd = {k: (None if k in null else t) for k, t in d.items()}
        oo = {k: (None if "out_" + k in null else t) for k, t in out.items()}
        for k in shift:
            if k.startswith("out_"):
                oo[k[4:]] = oo[k[4:]][1:]
            else:
                dd[k] = dd[k].reshape(-1)[1:]
        prm = _params(dict(sr.DEFAULTS, **dict(params))) if params is not None else None
        return _call(ctx_h, dd, oo, sizes, prm, intrinsics, size)

    assert call(ctx_h=None) == GH_ERR_ARG and call(params=None) == GH_ERR_ARG
    for sizes in ((-1, cap, P), (F, -1, P), (F, cap, -1), (1, 65536, P), (32769, 65535, P), (2**31 - 1, 1, P), (F, cap, 2**31 - 1 - F * cap),
                  (F, cap, 2**31 - 1)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for size in ((0, 480), (640, 0), (-1, 480), (640, -5)):
        assert call(size=size) == GH_ERR_ARG, size
    for intrinsics in ((0.0, 500.0, 320.0, 240.0), (500.0, 0.0, 320.0, 240.0), (-500.0, 500.0, 320.0, 240.0), (500.0, -1.0, 320.0, 240.0),
                       (nan, 500.0, 320.0, 240.0), (500.0, nan, 320.0, 240.0)):
        assert call(intrinsics=intrinsics) == GH_ERR_ARG, intrinsics
    for params in (dict(scale_factor=nan), dict(scale_factor=inf), dict(scale_factor=-inf), dict(scale_factor=0.999), dict(scale_factor=-1.2),
                   dict(n_levels=0), dict(n_levels=-1), dict(n_levels=33), dict(max_hamming=-1), dict(max_hamming=257),
                   dict(radius_near=-1e-300), dict(radius_far=-1.0), dict(radius_scale=-0.5)):
        assert call(params=params) == GH_ERR_ARG, params
    for k in ("radius_near", "radius_far", "near_cos", "radius_scale", "min_view_cos", "range_lo", "range_hi", "nn_ratio"):
        assert call(params={k: nan}) == GH_ERR_ARG, k
    for k in ("kps", "desc", "counts", "poses", "frame_search", "xyz", "views", "point_desc", "normal", "dist") + tuple("out_" + k for k in OUTPUTS):
        assert call(null=(k,)) == GH_ERR_ARG, k
    assert call(null=("row_point",)) == GH_ERR_ARG and call(null=("row_inlier",)) == GH_ERR_ARG  # both or neither
    for k in ("desc", "point_desc"):  # descriptors move as 32-bit words
        assert call(shift=(k,)) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: the optional inputs NULL, the bounds of the parameters, infinities
    for null, params in ((("node_point",), dict(scale_factor=1.0, n_levels=1)), (("row_point", "row_inlier"), dict(n_levels=32, max_hamming=0)),
                         (("status", "select"), dict(max_hamming=256, radius_near=0.0, radius_far=inf, radius_scale=0.0)),
                         (("node_point", "row_point", "row_inlier", "status", "select"),
                          dict(scale_factor=1e300, n_levels=2, range_lo=-inf, range_hi=inf, nn_ratio=inf, near_cos=-inf, min_view_cos=-inf))):
        assert call(null=null, params=params) == 0, null
    ctx.sync()
    assert not any((t[:-TAIL] == FILL).all().item() for t in out.values()) and all((t[-TAIL:] == FILL).all().item() for t in out.values())


def test_degenerate_sizes(ctx):
    import torch
    c = sc.soup()
    F, cap, P = _sizes(c)
    d = _inputs(c)
    prm = _params(c["params"])
    for sizes in ((0, cap, P), (F, 0, P)):  # no nodes: the totals only
        out = _dirty(F, cap)
        assert _call(ctx.h, d, out, sizes, prm) == 0
        torch.cuda.synchronize()
        assert _untouched(out, but=("totals",)) and _host(out, F, cap)["totals"].tolist() == [0] * 12, sizes
    # no points, or no searched frame: the node outputs fall through, every count is zero except the searched frames
    nothing = dict(d, frame_search=_dev(np.zeros(F, np.uint8)))
    n_searched = int((c["frame_search"] != 0).sum())
    rows = np.arange(cap)[None, :] < np.clip(c["counts"], 0, cap)[:, None]
    for dd, sizes, searched, name in ((d, (F, cap, 0), n_searched, "no points"), (nothing, (F, cap, P), 0, "no searched frame")):
        for claims in (True, False):
            e = dict(dd) if claims else dict(dd, row_point=None, row_inlier=None)
            out = _dirty(F, cap)
            assert _call(ctx.h, e, out, sizes, prm) == 0, name
            torch.cuda.synchronize()
            got = _host(out, F, cap)
            assert got["totals"].tolist() == [0] * 10 + [searched, 0] and not got["frame_totals"].any(), name
            assert (got["row_dist"] == 0xFFFF).all(), name
            if claims:
                assert got["row_point"].tolist() == c["row_point"].tolist() and got["row_inlier"].tolist() == (c["row_inlier"] != 0).tolist()
            else:
                assert got["row_point"].tolist() == np.where(rows.reshape(-1), sr.LOC_NO_POINT, sr.LOC_NO_ROW).tolist(), name
                assert not got["row_inlier"].any(), name
    # the restatement says the same
    for v in ((True, True, True, True), (True, False, True, True)):
        e = sr.search(**dict(sc.as_lists(c, *v), frame_search=[0] * F))
        assert e["totals"] == [0] * 12 and e["row_dist"] == [0xFFFF] * (F * cap)
        want = c["row_point"].tolist() if v[1] else np.where(rows.reshape(-1), sr.LOC_NO_POINT, sr.LOC_NO_ROW).tolist()
        assert e["row_point"] == want


SCENE_LEVELS, SCENE_SCALE = 8, 1.2
# The scene's cameras stand all around its points: a new frame sees a point from 82 to 143 degrees off the mean direction of the
# map frames (cosines -0.80 .. 0.14, worked out with the restatement), so with the default min_view_cos = 0.5 every pair that
# is not HELD ends as ANGLE.  The angle gate is opened for this scene; every other parameter is the default.
SCENE_PARAMS = dict(sr.DEFAULTS, min_view_cos=-1.0)


def scene_octaves(s):
    """Octaves that agree with the depth: a point is seen at octave 0 from the farthest frame that sees it, and one octave up
    for every factor 1.2 that a frame is closer (rounded, clamped to the pyramid)."""
    kps = s["kps"].copy()
    octave = np.zeros(kps.shape[:2], np.int32)
    tp = s["true_point"]
    centre = s["poses"][:, 4:]
    dist = np.linalg.norm(s["point_xyz_gt"][np.maximum(tp, 0)] - centre[:, None, :], axis=2)
    far = np.zeros(len(s["point_xyz_gt"]))
    np.maximum.at(far, tp[tp >= 0], dist[tp >= 0])
    o = np.rint(np.log(far[np.maximum(tp, 0)] / dist) / np.log(SCENE_SCALE))
    octave[tp >= 0] = np.clip(o[tp >= 0], 0, SCENE_LEVELS - 1).astype(np.int32)
    kps[..., 5] = octave.view(np.float32)
    return kps


def scene_search(s, kps, desc, poses, node_point, row_point, row_inlier, P1, xyz, status, d1, size):
    """The restatement on the scene's search call, from host arrays."""
    F = s["n_frames"]
    frame_search = np.zeros(F, np.uint8)
    frame_search[loc.SCENE_MAP:] = 1
    c = dict(n_frames=F, cap=s["cap"], kps=kps, desc=desc, counts=s["counts"], poses=poses, frame_search=frame_search,
             node_point=node_point, row_point=row_point, row_inlier=row_inlier, n_points=P1, xyz=xyz, status=status,
             select=np.ones(P1, np.uint8), views=d1["point_views"], point_desc=d1["point_desc"], normal=d1["point_normal"],
             dist=d1["point_dist"], intrinsics=s["intrinsics"], size=size, params=SCENE_PARAMS)
    return sr.search(**sc.as_lists(c, use_select=False))


def test_the_search_recovers_rows_that_the_pair_matches_lost(ctx):
    """localize_cases.scene() through track_extend_cases.scene() (which knows the true point behind every row), descriptors
    behind every row as tests/test_point_describe_gpu.py makes them, octaves that agree with the depth: link_tracks ->
    triangulate_tracks -> describe_points -> localize_pairs -> search_projection in place on localize's claims, with its poses
    for the new frames -> extend_tracks; nothing is read back before the last call has been issued.  A PLANTED row is a keypoint
    of a new frame that every pair match sends to a wrong point: the PnP turns the correspondence down, and the row stays
    without a point although its true point is in the map and projects onto it.  Asserted: the search equals the restatement;
    every row it added carries its true point; at least one planted row comes back with its true point; extend_tracks adopts more
    nodes than it does on localize's claims alone.  Printed: the pairs per verdict and the planted rows recovered."""
    import torch
    from gslam_amd import estimator
    s = ec.scene(False)
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    P1 = N // 2
    size = (int(2 * s["intrinsics"][2]), int(2 * s["intrinsics"][3]))
    kps_host, desc_host = scene_octaves(s), _scene_desc(s)
    kps, counts, desc, poses1 = _dev(kps_host), _dev(s["counts"]), _dev(desc_host), _dev(s["poses"])
    frame_search = torch.zeros(F, dtype=torch.uint8, device="cuda")
    frame_search[loc.SCENE_MAP:] = 1
    link = estimator.link_tracks(ctx, kps, counts, _dev(s["map_q"]), _dev(s["map_t"]), _dev(s["map_idx1"]), None, s["intrinsics"])
    tri = estimator.triangulate_tracks(ctx, poses1, link["obs_cam"], link["obs_point"], link["obs_xy"], P1)
    d1 = estimator.describe_points(ctx, kps, desc, counts, poses1, link["obs_cam"], link["obs_point"], link["obs_node"], P1,
                                   tri["point_xyz"], obs_use=tri["obs_good"], point_status=tri["status"])
    locz = estimator.localize_pairs(ctx, kps, counts, _dev(s["new_q"]), _dev(s["new_t"]), _dev(s["new_idx1"]), None, link["node_point"],
                                    tri["point_xyz"], tri["status"], s["intrinsics"], ransac_threshold=loc.SCENE_RANSAC_THRESHOLD,
                                    seed=loc.SCENE_SEED, inlier_threshold=loc.SCENE_INLIER_THRESHOLD)
    ext = lambda rp, ri: estimator.extend_tracks(ctx, kps, counts, _dev(s["ext_q"]), _dev(s["ext_t"]), _dev(s["ext_idx1"]), None,
                                                 link["node_point"], P1, rp, ri, s["intrinsics"])
    claims0 = locz["row_point"].clone(), locz["row_inlier"].clone()
    ext0 = ext(*claims0)
    poses2 = poses1.clone()
    poses2[loc.SCENE_MAP:] = locz["poses"][loc.SCENE_MAP:]
    found = estimator.search_projection(ctx, kps, desc, counts, poses2, frame_search, P1, tri["point_xyz"], d1, s["intrinsics"], size,
                                        node_point=link["node_point"], row_point=locz["row_point"], row_inlier=locz["row_inlier"],
                                        point_status=tri["status"], params=_params(SCENE_PARAMS), in_place=True)
    ext1 = ext(found["row_point"], found["row_inlier"])
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    assert found["row_point"].data_ptr() == locz["row_point"].data_ptr() and found["row_inlier"].data_ptr() == locz["row_inlier"].data_ptr()

    e = scene_search(s, kps_host, desc_host, host(poses2), host(link["node_point"]), host(claims0[0]), host(claims0[1]), P1,
                     host(tri["point_xyz"]), host(tri["status"]), {k: host(v) for k, v in d1.items()}, size)
    got = {k: host(found[k]) for k in OUTPUTS}
    _assert_same(got, sc.as_arrays(e, F), "scene")

    node_point, true_point = host(link["node_point"]), s["true_point"].reshape(-1)
    truth = {int(p): int(t) for p, t in zip(node_point, true_point) if p >= 0}  # map point id -> the graph's point
    added = np.flatnonzero(got["row_dist"] != 0xFFFF)
    assert len(added) > 0 and all(truth[int(got["row_point"][n])] == true_point[n] for n in added)
    assert (got["row_inlier"][added] == 1).all() and (host(claims0[1])[added] == 0).all()
    planted = np.flatnonzero(s["planted"].reshape(-1))
    recovered = [n for n in planted if got["row_dist"][n] != 0xFFFF]
    per = collections.Counter(e["verdict"].values())
    print("pairs per verdict:", ", ".join("%s %d" % (sr.VERDICTS[k], per[k]) for k in sorted(per)), "; rows added %d, planted rows %d, "
          "recovered %d; extend adopts %d nodes with the search and %d without" %
          (len(added), len(planted), len(recovered), host(ext1["totals"])[2], host(ext0["totals"])[2]))
    assert len(recovered) >= 1
    assert host(ext1["totals"])[2] > host(ext0["totals"])[2]
