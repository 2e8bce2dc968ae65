"""GPU parity of gh_describe_points_dev with the plain-Python restatement tests/point_describe_restate.py, byte for byte, on the
inputs of tests/point_describe_cases.py (tests/test_point_describe_cpu.py shows what they reach) in all eight NULL-variants
(obs_use, status, select); two runs; the argument contract; the degenerate sizes; then the call in its place on
localize_cases.scene(): link -> triangulate -> describe, then localize -> extend -> triangulate the new points -> describe what
changed, without a read-back in between.  Every output buffer goes in with every byte 0xA5 and 16 bytes longer than its
capacity, so that an entry left out, a SKIPPED entry that was written and a write past the end all show."""
import ctypes as C
import itertools

import numpy as np
import pytest

import localize_cases as loc
import point_describe_cases as pc
import point_describe_restate as pr
import track_extend_cases as ec

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS, DTYPE = pc.OUTPUTS, pc.DTYPE
TAIL = 16
FILL = loc.FILL
VARIANTS = list(itertools.product((True, False), (True, False), (True, False)))  # obs_use, status, select
CASES = {c["name"]: c for c in pc.cases()}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(n_points):
    return dict(point_state=n_points, point_desc=32 * n_points, point_obs=8 * n_points, point_views=4 * n_points,
                point_normal=24 * n_points, point_dist=16 * n_points, totals=16)


def _dirty(n_points):
    import torch
    return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in _bytes(n_points).items()}


def _before(n_points):
    """What _dirty holds, as host arrays at capacity."""
    return {k: np.full(n, FILL, np.uint8).view(DTYPE[k]) for k, n in _bytes(n_points).items()}


def _untouched(out, but=()):
    return all((t == FILL).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_obs_use=True, use_status=True, use_select=True):
    d = {k: _dev(c[k]) for k in ("kps", "desc", "counts", "poses", "obs_cam", "obs_point", "obs_node", "xyz")}
    d["obs_use"] = _dev(c["obs_use"]) if use_obs_use else None
    d["status"] = _dev(c["status"]) if use_status else None
    d["select"] = _dev(c["select"]) if use_select else None
    return d


def _params(c):
    from gslam_amd import hip
    return hip.PointDescParams(c["scale_factor"], c["n_levels"], c["max_views"])


def _call(ctx_h, d, out, sizes, params):
    from gslam_amd import hip
    F, cap, n_obs, n_points = sizes
    return hip.lib.gh_describe_points_dev(ctx_h, _ptr(d["kps"]), _ptr(d["desc"]), _ptr(d["counts"]), F, cap, _ptr(d["poses"]),
                                          _ptr(d["obs_cam"]), _ptr(d["obs_point"]), _ptr(d["obs_node"]), _ptr(d["obs_use"]), n_obs,
                                          n_points, _ptr(d["xyz"]), _ptr(d["status"]), _ptr(d["select"]),
                                          C.byref(params) if params is not None else None, *(_ptr(out[k]) for k in OUTPUTS))


def _sizes(c):
    return c["n_frames"], c["cap"], len(c["obs_point"]), c["n_points"]


def _host(out, n_points):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k, n in _bytes(n_points).items():
        raw = out[k].cpu().numpy()
        assert (raw[n:] == FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(DTYPE[k])
    return got


def _run(ctx, c, use_obs_use=True, use_status=True, use_select=True):
    """gh_describe_points_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    out = _dirty(c["n_points"])
    st = _call(ctx.h, _inputs(c, use_obs_use, use_status, use_select), out, _sizes(c), _params(c))
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return _host(out, c["n_points"])


def _assert_same(got, want, name, note=()):
    assert got["totals"].tolist() == want["totals"].tolist(), (name, note, got["totals"], want["totals"])
    for k in OUTPUTS:
        g, w = got[k].reshape(-1), want[k].reshape(-1)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint8) != w.view(np.uint8)) // g.dtype.itemsize // pc.WIDTH.get(k, 1)
            raise AssertionError((name, note, k, "points", sorted(set(bad.tolist()))[:10]))


@pytest.mark.parametrize("name", list(CASES))
def test_cases_match_the_restatement_byte_for_byte(ctx, name):
    c = CASES[name]
    P = c["n_points"]
    for v in VARIANTS:
        e = pc.restate(c, *v)
        want = pc.as_arrays(e, P, _before(P))
        got = _run(ctx, c, *v)
        _assert_same(got, want, name, v)
        skipped = np.flatnonzero(got["point_state"] == pr.SKIPPED)
        assert (len(skipped) > 0) == (v[2] and (c["select"] == 0).any())
        for k in ("point_desc", "point_obs", "point_views", "point_normal", "point_dist"):  # SKIPPED entries are still 0xA5
            assert (got[k].reshape(P, -1)[skipped].view(np.uint8) == FILL).all(), (name, v, k)


def test_two_runs_give_equal_bytes(ctx):
    for c in (pc.soup(64), pc.long_track(), pc.centre()):
        a, b = _run(ctx, c), _run(ctx, c)
        assert all(a[k].tobytes() == b[k].tobytes() for k in OUTPUTS), c["name"]


def test_argument_errors_leave_the_outputs_alone(ctx):
    from gslam_amd import hip
    c = pc.soup(64)
    F, cap, n_obs, P = _sizes(c)
    d = _inputs(c)
    out = _dirty(P)
    nan, inf = float("nan"), float("inf")

    def call(ctx_h=ctx.h, sizes=(F, cap, n_obs, P), params=(1.2, 8, 64), null=(), shift=()):
        dd = {k: (None if k in null else t) for k, t in d.items()}
        oo = {k: (None if "out_" + k in null else t) for k, t in out.items()}
        for k in shift:
            if k.startswith("out_"):
                oo[k[4:]] = oo[k[4:]][1:]
            else:
                dd[k] = dd[k].reshape(-1)[1:]
        return _call(ctx_h, dd, oo, sizes, hip.PointDescParams(*params) if params is not None else None)

    assert call(ctx_h=None) == GH_ERR_ARG and call(params=None) == GH_ERR_ARG
    for sizes in ((-1, cap, n_obs, P), (F, -1, n_obs, P), (F, cap, -1, P), (F, cap, n_obs, -1), (1, 65536, n_obs, P),
                  (32769, 65535, n_obs, P), (2**31 - 1, 1, n_obs, P), (F, cap, n_obs, 2**31 - 1 - F * cap), (F, cap, n_obs, 2**31 - 1)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for params in ((nan, 8, 64), (inf, 8, 64), (-inf, 8, 64), (0.999, 8, 64), (-1.2, 8, 64), (1.2, 0, 64), (1.2, -1, 64), (1.2, 33, 64),
                   (1.2, 8, 0), (1.2, 8, -1), (1.2, 8, 65)):
        assert call(params=params) == GH_ERR_ARG, params
    for k in ("kps", "desc", "counts", "poses", "obs_cam", "obs_point", "obs_node", "xyz") + tuple("out_" + k for k in OUTPUTS):
        assert call(null=(k,)) == GH_ERR_ARG, k
    for k in ("desc", "out_point_desc"):  # descriptors move as 32-bit words
        assert call(shift=(k,)) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: the three optional inputs NULL, the bounds of the parameters
    for null, params in ((("obs_use",), (1.2, 8, 64)), (("status",), (1.0, 1, 1)), (("select",), (1.2, 32, 64)),
                         (("obs_use", "status", "select"), (1e300, 2, 9))):
        assert call(null=null, params=params) == 0, null
    ctx.sync()
    assert not any((t[:-TAIL] == FILL).all().item() for t in out.values()) and all((t[-TAIL:] == FILL).all().item() for t in out.values())


def test_degenerate_sizes(ctx):
    import torch
    c = pc.soup(64)
    F, cap, n_obs, P = _sizes(c)
    d = _inputs(c)
    out = _dirty(P)  # no points: the totals only
    assert _call(ctx.h, d, out, (F, cap, n_obs, 0), _params(c)) == 0
    torch.cuda.synchronize()
    assert _untouched(out, but=("totals",)) and _host(out, 0)["totals"].tolist() == [0] * 4
    # no observations, no frames, no rows: every selected usable point is EMPTY
    for sizes, name in (((F, cap, 0, P), "no_obs"), ((0, cap, n_obs, P), "no_frames"), ((F, 0, n_obs, P), "no_rows")):
        out = _dirty(P)
        assert _call(ctx.h, d, out, sizes, _params(c)) == 0, name
        torch.cuda.synchronize()
        got = _host(out, P)
        want_state = np.where(c["select"] == 0, pr.SKIPPED, np.where(c["status"] != 0, pr.NOT_OK, pr.EMPTY))
        assert got["point_state"].tolist() == want_state.tolist(), name
        n_empty, n_not_ok = int((want_state == pr.EMPTY).sum()), int((want_state == pr.NOT_OK).sum())
        assert got["totals"].tolist() == [0, n_empty, n_not_ok, 0], name
        written = want_state != pr.SKIPPED
        assert (got["point_obs"].reshape(P, 2)[written] == -1).all() and not got["point_views"][written].any()
        assert not got["point_desc"].reshape(P, 32)[written].any() and not got["point_normal"].view(np.uint8).reshape(P, 24)[written].any()
        assert not got["point_dist"].view(np.uint8).reshape(P, 16)[written].any()
        assert (got["point_desc"].reshape(P, 32)[~written] == FILL).all()
    e = dict(c, obs_cam=c["obs_cam"][:0], obs_point=c["obs_point"][:0], obs_node=c["obs_node"][:0], obs_use=c["obs_use"][:0], name="no_obs")
    _assert_same(got, pc.as_arrays(pc.restate(e), P, _before(P)), "no_obs")


def _scene_desc(s, seed=31):
    """Descriptors for the scene's rows, seeded: one base per true point, up to 59 bits flipped per keypoint; noise elsewhere."""
    rng = np.random.default_rng(seed)
    F, cap = s["n_frames"], s["cap"]
    base = rng.integers(0, 256, size=(150, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, size=(F, cap, 32), dtype=np.uint8)
    for f, i in zip(*np.nonzero(s["true_point"] >= 0)):
        desc[f, i] = pc._flip(rng, base[s["true_point"][f, i]], int(rng.integers(0, pc.MAX_FLIPS + 1)))
    return desc


def _restate_map(s, desc, poses, obs, obs_use, n_points, xyz, status, select):
    c = dict(name="scene", n_frames=s["n_frames"], cap=s["cap"], kps=s["kps"], desc=desc, counts=s["counts"], poses=poses,
             obs_cam=obs["obs_cam"], obs_point=obs["obs_point"], obs_node=obs["obs_node"],
             obs_use=obs_use if obs_use is not None else np.ones(len(obs["obs_cam"]), np.uint8), n_points=n_points, xyz=xyz,
             status=status, select=select if select is not None else np.ones(n_points, np.uint8), scale_factor=1.2, n_levels=8,
             max_views=64)
    return pr.describe(**pc.as_lists(c, use_select=select is not None))


@pytest.mark.parametrize("late_points", [False, True])
def test_the_map_is_described_and_refreshed_without_a_read_back(ctx, late_points):
    """localize_cases.scene() (through track_extend_cases.scene(), which adds the pairs among the new frames and the true point
    behind every row): link_tracks -> triangulate_tracks -> describe_points with the padded arrays (n_obs = N, n_points = N / 2,
    status and obs_good from the triangulation); then localize_pairs -> extend_tracks -> triangulate_tracks of the new points
    -> describe_points with point_select = point_new | point_grew into the arrays of the first call.  Nothing is read back
    before the last call has been issued.  Both calls equal the restatement byte for byte; the old points that neither grew
    nor are new keep their bytes from the first call; the grown points show more views.  (The second call takes no obs_use:
    extend_tracks renumbers the observations, and the scene is free of noise, so the first triangulation dropped none.)
    Printed, not asserted: the largest median distance of a chosen descriptor and the smallest cosine between an observation's
    ray and its point's direction."""
    import torch
    from gslam_amd import estimator
    s = ec.scene(late_points)
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    P1, PC = N // 2, N // 2 + N // 2
    desc_host = _scene_desc(s)
    kps, counts, desc, poses1 = _dev(s["kps"]), _dev(s["counts"]), _dev(desc_host), _dev(s["poses"])
    link = estimator.link_tracks(ctx, kps, counts, _dev(s["map_q"]), _dev(s["map_t"]), _dev(s["map_idx1"]), None, s["intrinsics"])
    tri = estimator.triangulate_tracks(ctx, poses1, link["obs_cam"], link["obs_point"], link["obs_xy"], P1)
    d1 = estimator.describe_points(ctx, kps, desc, counts, poses1, link["obs_cam"], link["obs_point"], link["obs_node"], P1,
                                   tri["point_xyz"], obs_use=tri["obs_good"], point_status=tri["status"])
    locz = estimator.localize_pairs(ctx, kps, counts, _dev(s["new_q"]), _dev(s["new_t"]), _dev(s["new_idx1"]), None, link["node_point"],
                                    tri["point_xyz"], tri["status"], s["intrinsics"], ransac_threshold=loc.SCENE_RANSAC_THRESHOLD,
                                    seed=loc.SCENE_SEED, inlier_threshold=loc.SCENE_INLIER_THRESHOLD)
    ext = estimator.extend_tracks(ctx, kps, counts, _dev(s["ext_q"]), _dev(s["ext_t"]), _dev(s["ext_idx1"]), None, link["node_point"], P1,
                                  locz["row_point"], locz["row_inlier"], s["intrinsics"])
    poses2 = poses1.clone()
    poses2[loc.SCENE_MAP:] = locz["poses"][loc.SCENE_MAP:]
    xyz = torch.zeros((PC, 3), dtype=torch.float64, device="cuda")
    xyz[:P1] = tri["point_xyz"]
    tri2 = estimator.triangulate_tracks(ctx, poses2, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], PC, point_select=ext["point_new"],
                                        point_xyz=xyz)
    status2 = torch.full((PC,), estimator.TRACK_TOO_FEW, dtype=torch.int32, device="cuda")
    status2[:P1] = tri["status"]
    status2 = torch.where(ext["point_new"] != 0, tri2["status"], status2)  # (that call marks what it skips SKIPPED: keep the map's)
    select2 = ext["point_new"] | ext["point_grew"]
    grown = {k: torch.cat([d1[k], torch.zeros((PC - P1,) + tuple(d1[k].shape[1:]), dtype=d1[k].dtype, device="cuda")])
             for k in estimator.DESCRIBE_OUTPUTS if k != "totals"}
    grown["totals"] = torch.zeros(4, dtype=torch.int32, device="cuda")
    grown = {k: grown[k] for k in estimator.DESCRIBE_OUTPUTS}
    first = {k: d1[k].clone() for k in d1}
    d2 = estimator.describe_points(ctx, kps, desc, counts, poses2, ext["obs_cam"], ext["obs_point"], ext["obs_node"], PC,
                                   tri2["point_xyz"], point_status=status2, point_select=select2, out=grown)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    assert all(d2[k].data_ptr() == grown[k].data_ptr() for k in grown)

    obs1 = {k: host(link[k]) for k in ("obs_cam", "obs_point", "obs_node")}
    e1 = _restate_map(s, desc_host, s["poses"], obs1, host(tri["obs_good"]), P1, host(tri["point_xyz"]), host(tri["status"]), None)
    got1 = {k: host(first[k]) for k in OUTPUTS}
    _assert_same(got1, pc.as_arrays(e1, P1), "scene: first call")
    assert e1["totals"][0] >= 50 and e1["totals"][2] > 0  # the map's points; the padding past them is NOT_OK

    obs2 = {k: host(ext[k]) for k in ("obs_cam", "obs_point", "obs_node")}
    sel = host(select2)
    e2 = _restate_map(s, desc_host, host(poses2), obs2, None, PC, host(tri2["point_xyz"]), host(status2), sel)
    before = {k: np.concatenate([got1[k].reshape(P1, -1), np.zeros((PC - P1, pc.WIDTH[k]), DTYPE[k])]) for k in pc.WIDTH}
    got2 = {k: host(d2[k]) for k in OUTPUTS}
    _assert_same(got2, pc.as_arrays(e2, PC, before), "scene: second call")
    untouched = np.flatnonzero(sel[:P1] == 0)
    grew = np.flatnonzero(host(ext["point_grew"]) != 0)
    new = np.flatnonzero(host(ext["point_new"]) != 0)
    assert len(untouched) > 0 and len(grew) >= 50 and (len(new) >= 20 if late_points else len(new) == 0)
    assert (got2["point_state"][untouched] == pr.SKIPPED).all()
    for k in pc.WIDTH:
        if k != "point_state":
            assert got2[k].reshape(PC, -1)[untouched].tobytes() == got1[k].reshape(P1, -1)[untouched].tobytes(), k
    ok_grew = grew[host(status2)[grew] == estimator.TRACK_OK]
    assert len(ok_grew) >= 50 and (got2["point_views"][ok_grew] > got1["point_views"][ok_grew]).all()
    if late_points:
        new_ok = new[got2["point_state"][new] == pr.OK]
        assert len(new_ok) > 0 and (got2["point_views"][new_ok] >= 2).all()

    cos = []
    ok = np.flatnonzero(got2["point_state"] == pr.OK)
    xyz2, p2 = host(tri2["point_xyz"]), host(poses2)
    for p in ok:
        for k in e2["tracks"][p]:
            v = xyz2[p] - p2[obs2["obs_node"][k] // cap, 4:]
            cos.append(float(v @ got2["point_normal"].reshape(PC, 3)[p] / np.linalg.norm(v)))
    print("late_points %s: %d + %d points described, %d refreshed; largest median distance of a chosen descriptor %d; smallest "
          "cosine between an observation's ray and its point's direction %.4f" %
          (late_points, e1["totals"][0], len(new), int(sel.sum()), max(list(e1["med"].values()) + list(e2["med"].values())), min(cos)))
