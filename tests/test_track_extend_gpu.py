"""GPU parity of gh_extend_tracks_dev with the plain-Python restatement tests/track_extend_restate.py, byte for byte, on the
inputs of tests/track_extend_cases.py (tests/test_track_extend_cpu.py shows what they reach): the census (and with it the input
of tests/map_wide_cases.py, more than 1024 * 256 nodes), a point adopted from
256 frames, a new track through 64 frames and a random growing map in three pair orders, a random soup at N = 512 and N = 513;
the device against gh_link_tracks_dev where the contract says they agree; the argument contract; then the call in its place:
link -> triangulate -> localize -> extend -> triangulate the new points, without a read-back in between.  Every output buffer
goes in with every byte 0xA5 and 16 bytes longer than its capacity, so that an entry left out and a write past the end both
show."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as loc
import map_wide_cases as wide
import track_extend_cases as ec
import track_extend_restate as er
import track_link_cases as lc
import tracks_restate as tr

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS = ec.OUTPUTS
DTYPE = dict(node_point=np.int32, obs_cam=np.int32, obs_point=np.int32, obs_xy=np.float64, obs_node=np.int32, point_len=np.int32,
             point_new=np.uint8, point_grew=np.uint8, totals=np.int32)
LINK_OUT = ("node_point", "obs_cam", "obs_point", "obs_xy", "obs_node", "point_len", "totals")
TAIL = 16
FILL = loc.FILL


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(N, n_points):
    PC = n_points + N // 2
    return dict(node_point=4 * N, obs_cam=4 * N, obs_point=4 * N, obs_xy=16 * N, obs_node=4 * N, point_len=4 * PC, point_new=PC,
                point_grew=PC, totals=24)


def _dirty(N, n_points):
    import torch
    return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in _bytes(N, n_points).items()}


def _untouched(out, but=()):
    return all((t == FILL).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_inlier=True, use_map=True, use_claims=True):
    d = {k: _dev(c[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1")}
    d["inlier"] = _dev(c["inlier"]) if use_inlier else None
    d["node_point_in"] = _dev(c["node_point"]) if use_map else None
    d["row_point"] = _dev(c["row_point"]) if use_claims else None
    d["row_inlier"] = _dev(c["row_inlier"]) if use_claims else None
    for k in ("pair_q", "pair_t", "idx1"):  # (an empty tensor has no storage)
        if d[k].numel() == 0:
            d[k] = None
    return d


def _call(ctx_h, d, out, sizes, min_views, intrinsics=ec.INTRINSICS):
    from gslam_amd import hip
    F, cap, P, n_points = sizes
    return hip.lib.gh_extend_tracks_dev(ctx_h, _ptr(d["kps"]), _ptr(d["counts"]), F, cap, _ptr(d["pair_q"]), _ptr(d["pair_t"]), P,
                                        _ptr(d["idx1"]), _ptr(d["inlier"]), _ptr(d["node_point_in"]), n_points, _ptr(d["row_point"]),
                                        _ptr(d["row_inlier"]), *(C.c_double(v) for v in intrinsics), min_views,
                                        *(_ptr(out[k]) for k in OUTPUTS))


def _sizes(c):
    return c["n_frames"], c["cap"], len(c["pair_q"]), c["n_points"]


def _host(out, N, n_points):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k, n in _bytes(N, n_points).items():
        raw = out[k].cpu().numpy()
        assert (raw[n:] == FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(DTYPE[k])
    got["obs_xy"] = got["obs_xy"].reshape(-1, 2)
    return got


def _run(ctx, c, use_inlier=True, use_map=True, use_claims=True, min_views=None):
    """gh_extend_tracks_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    N = c["n_frames"] * c["cap"]
    out = _dirty(N, c["n_points"])
    st = _call(ctx.h, _inputs(c, use_inlier, use_map, use_claims), out, _sizes(c), c["min_views"] if min_views is None else min_views)
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return _host(out, N, c["n_points"])


def _assert_same(got, e, c):
    N = c["n_frames"] * c["cap"]
    want = ec.as_arrays(e, N, c["n_points"] + N // 2)
    assert got["totals"].tolist() == want["totals"].tolist(), (c["name"], got["totals"], want["totals"])
    assert got["node_point"].tolist() == want["node_point"].tolist(), c["name"]
    assert got["point_len"].tolist() == want["point_len"].tolist(), c["name"]
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (c["name"], k)


VARIANTS = [(True, True, True), (False, True, True), (True, True, False), (True, False, True)]  # inlier bytes, map, claims


@pytest.mark.parametrize("min_views", [3, 2])
@pytest.mark.parametrize("use_inlier,use_map,use_claims", VARIANTS)
def test_census_matches_the_restatement_byte_for_byte(ctx, use_inlier, use_map, use_claims, min_views):
    c = ec.census()
    _assert_same(_run(ctx, c, use_inlier, use_map, use_claims, min_views), ec.restate(c, use_inlier, use_map, use_claims, min_views), c)
    c = wide.extend_case()  # N + 1 > 1024 * 256: the second trip through the loop of ext_flags, with verdicts to count in it
    _assert_same(_run(ctx, c, use_inlier, use_map, use_claims, min_views), wide.extend_restated(use_inlier, use_map, use_claims, min_views), c)


@pytest.mark.parametrize("mapped_in_frame_128", [False, True])
def test_one_point_adopted_from_256_frames(ctx, mapped_in_frame_128):
    c = ec.hub(mapped_in_frame_128)
    first = None
    for order in ("forward", "reversed", "shuffled"):
        got = _run(ctx, ec.reorder(c, order, seed=3))
        _assert_same(got, ec.restate(c), c)
        first = first or got
        assert all(got[k].tobytes() == first[k].tobytes() for k in OUTPUTS), order
    assert got["totals"].tolist() == [514, 4, 255 if mapped_in_frame_128 else 256, 1 if mapped_in_frame_128 else 0, 0, 0]
    assert got["point_len"][:4].tolist() == [0, 257, 0, 257] and got["point_grew"][:3].tolist() == [0, 1, 0]
    for use_inlier, use_map, use_claims in VARIANTS[1:]:
        _assert_same(_run(ctx, c, use_inlier, use_map, use_claims), ec.restate(c, use_inlier, use_map, use_claims), c)


def test_new_track_through_64_frames_in_any_pair_order_gives_the_same_bytes(ctx):
    c = ec.chain()
    e, first = ec.restate(c), None
    for order in ("forward", "reversed", "shuffled"):
        got = _run(ctx, ec.reorder(c, order, seed=3))
        _assert_same(got, e, c)
        assert got["totals"].tolist() == [196, 4, 64, 0, 0, 0] and got["point_len"][:4].tolist() == [66, 0, 66, 64]
        first = first or got
        for k in OUTPUTS:
            assert got[k].tobytes() == first[k].tobytes(), (order, k)
    for use_inlier, use_map, use_claims in VARIANTS[1:]:
        _assert_same(_run(ctx, c, use_inlier, use_map, use_claims), ec.restate(c, use_inlier, use_map, use_claims), c)


@pytest.mark.parametrize("use_inlier", [True, False])
def test_random_growth_in_any_pair_order_gives_the_same_bytes(ctx, use_inlier):
    c, with_inlier, without = ec.random_case()
    e = with_inlier if use_inlier else without
    assert e["totals"][1] - c["n_points"] >= 5 and min(e["totals"][2:5]) >= 1
    first = None
    for order in ("forward", "reversed", "shuffled"):
        got = _run(ctx, ec.reorder(c, order, seed=4), use_inlier)
        _assert_same(got, e, c)
        first = first or got
        for k in OUTPUTS:
            assert got[k].tobytes() == first[k].tobytes(), (order, k)
    if use_inlier:
        _assert_same(_run(ctx, c, True, True, False), ec.restate(c, True, True, False), c)
        _assert_same(_run(ctx, c, True, False, True), ec.restate(c, True, False, True), c)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("use_inlier,use_map,use_claims", VARIANTS)
def test_block_boundaries(ctx, which, use_inlier, use_map, use_claims):
    c = ec.boundaries()[which]
    assert c["n_frames"] * c["cap"] == (512, 513)[which]
    for mv in (2, 3):
        _assert_same(_run(ctx, c, use_inlier, use_map, use_claims, mv), ec.restate(c, use_inlier, use_map, use_claims, mv), c)


def _link(ctx, c, use_inlier, min_views):
    """gh_link_tracks_dev on the same device arrays -> dict of host arrays."""
    import torch
    from gslam_amd import hip
    N = c["n_frames"] * c["cap"]
    sizes = dict(node_point=4 * N, obs_cam=4 * N, obs_point=4 * N, obs_xy=16 * N, obs_node=4 * N, point_len=4 * (N // 2), totals=16)
    out = {k: torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    d = _inputs(dict(c, node_point=np.zeros(1, np.int32), row_point=np.zeros(1, np.int32), row_inlier=np.zeros(1, np.uint8)), use_inlier)
    fx, fy, cx, cy = ec.INTRINSICS
    st = hip.lib.gh_link_tracks_dev(ctx.h, _ptr(d["kps"]), _ptr(d["counts"]), c["n_frames"], c["cap"], _ptr(d["pair_q"]), _ptr(d["pair_t"]),
                                    len(c["pair_q"]), _ptr(d["idx1"]), _ptr(d["inlier"]), C.c_double(fx), C.c_double(fy), C.c_double(cx),
                                    C.c_double(cy), min_views, *(_ptr(out[k]) for k in LINK_OUT))
    assert st == 0
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().view(DTYPE[k]) for k in LINK_OUT}


def test_without_a_map_and_claims_it_equals_gh_link_tracks_dev(ctx):
    """The device against the device: no restatement takes part."""
    for c in lc.census() + [lc.random_case()[0], lc.chain("shuffled", seed=3), lc.hub(True)] + ec.boundaries():
        N = c["n_frames"] * c["cap"]
        for use_inlier in (True, False):
            want = _link(ctx, c, use_inlier, c["min_views"])
            bare = dict(c, n_points=0, node_point=np.full(N, 3, np.int32), row_point=None, row_inlier=None)
            for use_map in (False, True):  # NULL, and a map array with n_points == 0: every value in it means "no point"
                got = _run(ctx, bare, use_inlier, use_map, False)
                for k in LINK_OUT[:-1]:
                    assert got[k].reshape(-1).tobytes() == want[k].tobytes(), (c["name"], use_inlier, use_map, k)
                assert got["totals"].tolist() == [want["totals"][0], want["totals"][1], 0, 0, want["totals"][2], want["totals"][3]]
                assert not got["point_grew"].any() and got["point_new"].tolist() == [1] * want["totals"][1] + [0] * (N // 2 - want["totals"][1])


def test_argument_errors_leave_the_outputs_alone(ctx):
    c = ec.census()
    F, cap, P, n_points = _sizes(c)
    d = _inputs(c)
    out = _dirty(F * cap, n_points)
    nan = float("nan")

    def call(ctx_h=ctx.h, sizes=(F, cap, P, n_points), min_views=2, intrinsics=ec.INTRINSICS, null=()):
        dd = {k: (None if k in null else t) for k, t in d.items()}
        oo = {k: (None if k in null else t) for k, t in out.items()}
        return _call(ctx_h, dd, oo, sizes, min_views, intrinsics)

    assert call(ctx_h=None) == GH_ERR_ARG
    for sizes in ((-1, cap, P, n_points), (F, -1, P, n_points), (F, cap, -1, n_points), (F, cap, P, -1), (1, 65536, P, n_points),
                  (32769, 65535, P, n_points), (2**31 - 1, 1, P, n_points), (F, cap, P, 2**31 - 1 - F * cap),
                  (F, cap, P, 2**31 - 1), (32768, 65535, P, 2**31 - 1 - 32768 * 65535)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for mv in (1, 0, -3):
        assert call(min_views=mv) == GH_ERR_ARG, mv
    fx, fy, cx, cy = ec.INTRINSICS
    for bad in ((0.0, fy), (-1.0, fy), (nan, fy), (fx, 0.0), (fx, -2.0), (fx, nan)):
        assert call(intrinsics=bad + (cx, cy)) == GH_ERR_ARG, bad
    for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "row_point", "row_inlier") + OUTPUTS:
        assert call(null=(k,)) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: no inlier bytes, no map, no claims
    for null in (("inlier",), ("node_point_in",), ("row_point", "row_inlier")):
        assert call(null=null) == 0, null
    ctx.sync()
    assert not any((t[:-TAIL] == FILL).all().item() for t in out.values()) and all((t[-TAIL:] == FILL).all().item() for t in out.values())


def test_degenerate_sizes(ctx):
    import torch
    c = ec.census()
    d = _inputs(c)
    F, cap, P, n_points = _sizes(c)
    for f, k in ((0, cap), (F, 0), (0, 0)):  # N == 0: totals and the n_points entries of the three point arrays
        out = _dirty(F * cap, n_points)
        assert _call(ctx.h, d, out, (f, k, P, n_points), 2) == 0
        torch.cuda.synchronize()
        assert _untouched(out, but=("point_len", "point_new", "point_grew", "totals"))
        assert out["totals"].cpu().numpy()[:24].view(np.int32).tolist() == [0, n_points, 0, 0, 0, 0] and (out["totals"][24:] == FILL).all().item()
        for name, size in (("point_len", 4), ("point_new", 1), ("point_grew", 1)):
            raw = out[name].cpu().numpy()
            assert not raw[:size * n_points].any() and (raw[size * n_points:] == FILL).all(), name
    out = _dirty(F * cap, n_points)  # N == 0 and n_points == 0: the totals only
    assert _call(ctx.h, d, out, (0, cap, P, 0), 2) == 0
    torch.cuda.synchronize()
    assert _untouched(out, but=("totals",)) and out["totals"].cpu().numpy()[:24].view(np.int32).tolist() == [0] * 6
    # no pairs: no new tracks, the adoptions stay; the pair arrays may be NULL then
    e = dict(c, pair_q=c["pair_q"][:0], pair_t=c["pair_t"][:0], idx1=c["idx1"][:0], inlier=c["inlier"][:0], name="no_pairs")
    got = _run(ctx, e, use_inlier=False)
    _assert_same(got, ec.restate(e, False), e)
    assert got["totals"].tolist()[1:] == [n_points, 4, 8, 0, 0] and not got["point_new"].any()
    # no points: whatever the map and the claims hold, nobody is MAPPED and nobody claims
    e = dict(c, n_points=0, name="no_points")
    got = _run(ctx, e)
    _assert_same(got, ec.restate(e), e)
    assert got["totals"].tolist()[2:4] == [0, 0] and got["totals"][1] >= 1


def test_the_wrapper_refuses_a_tensor_a_kernel_could_not_read_before_any_launch(ctx):
    """estimator.extend_tracks with a float32 idx1, or with a transposed (non-contiguous) kps, raises ValueError naming the
    argument; nothing was launched, so every tensor that went in holds what it held.  F = 3, cap = 8, P = 2."""
    import torch
    from gslam_amd import estimator
    F, cap, P, n_points = 3, 8, 2, 5
    g = torch.Generator().manual_seed(7)
    good = dict(kps=torch.rand((F, cap, 7), generator=g).cuda(), counts=torch.full((F,), cap, dtype=torch.int32).cuda(),
                pair_q=torch.tensor([1, 2], dtype=torch.int32).cuda(), pair_t=torch.tensor([0, 1], dtype=torch.int32).cuda(),
                idx1=torch.randint(0, cap, (P, cap), generator=g, dtype=torch.int32).cuda(),
                inlier=torch.ones((P, cap), dtype=torch.uint8).cuda(),
                node_point=torch.randint(-1, n_points, (F * cap,), generator=g, dtype=torch.int32).cuda(),
                row_point=torch.randint(-1, n_points, (F * cap,), generator=g, dtype=torch.int32).cuda(),
                row_inlier=torch.ones(F * cap, dtype=torch.uint8).cuda())
    bad_idx1 = good["idx1"].to(torch.float32)
    bad_kps = torch.rand((F, 7, cap), generator=g).cuda().transpose(1, 2)
    assert tuple(bad_kps.shape) == (F, cap, 7) and not bad_kps.is_contiguous()
    for name, bad in (("idx1", bad_idx1), ("kps", bad_kps)):
        d = dict(good, **{name: bad})
        before = {k: t.clone() for k, t in d.items()}
        with pytest.raises(ValueError, match="^%s: " % name):
            estimator.extend_tracks(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["inlier"], d["node_point"],
                                    n_points, d["row_point"], d["row_inlier"], ec.INTRINSICS)
        torch.cuda.synchronize()
        for k, t in d.items():
            assert t.dtype == before[k].dtype and t.stride() == before[k].stride() and torch.equal(t, before[k]), (name, k)
    out = estimator.extend_tracks(ctx, *(good[k] for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "inlier", "node_point")),
                                  n_points, good["row_point"], good["row_inlier"], ec.INTRINSICS)  # (the same call, valid, goes through)
    torch.cuda.synchronize()
    assert out["totals"].numel() == 6


@pytest.mark.parametrize("late_points", [False, True])
def test_the_map_grows_by_three_frames_without_a_read_back(ctx, late_points):
    """localize_cases.scene(): link_tracks on the map pairs -> triangulate_tracks at the true poses -> localize_pairs for the 3 new
    frames -> extend_tracks with the new-versus-map pairs and exact pairs among the new frames -> triangulate_tracks of the new
    points only, at the poses localize_pairs found.  Nothing is read back before the last call has been issued.  Then the
    integer facts the scene was planted for, and every stage of the extension against its restatement byte for byte: the link,
    the first triangulation, the extension (on the row_point / row_inlier the device's localisation produced: the PnP chain has
    no restatement of its own, tests/test_localize_gpu.py holds it to the composition of the public pieces) and the second
    triangulation (on the poses of that localisation).
    In the scene as it stands every point is seen by at least three map frames, so the map holds all of them: the new frames
    adopt and nothing new may appear (a new track would be a second copy of a map point).  late_points takes every fourth point
    out of the map pairs, so that the map does not hold it and the new frames bring it in: there the new tracks, their
    triangulation at the poses the localisation found, and the hand-over of the extended map are not vacuous.
    The distance of the new OK points from the truth is printed, not asserted: there is no reference value for it.  Measured on
    an MI355X: see DESIGN.md 6i."""
    import torch
    from gslam_amd import estimator
    s = ec.scene(late_points)
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    n_map_pts = N // 2  # the capacity link_tracks leaves: ids past its n_points hold no observation and are TOO_FEW
    kps, counts = _dev(s["kps"]), _dev(s["counts"])
    link = estimator.link_tracks(ctx, kps, counts, _dev(s["map_q"]), _dev(s["map_t"]), _dev(s["map_idx1"]), None, s["intrinsics"])
    tri = estimator.triangulate_tracks(ctx, _dev(s["poses"]), link["obs_cam"], link["obs_point"], link["obs_xy"], n_map_pts)
    locz = estimator.localize_pairs(ctx, kps, counts, _dev(s["new_q"]), _dev(s["new_t"]), _dev(s["new_idx1"]), None, link["node_point"],
                                    tri["point_xyz"], tri["status"], s["intrinsics"], ransac_threshold=loc.SCENE_RANSAC_THRESHOLD,
                                    seed=loc.SCENE_SEED, inlier_threshold=loc.SCENE_INLIER_THRESHOLD)
    ext_q, ext_t, ext_idx1 = _dev(s["ext_q"]), _dev(s["ext_t"]), _dev(s["ext_idx1"])
    ext = estimator.extend_tracks(ctx, kps, counts, ext_q, ext_t, ext_idx1, None, link["node_point"], n_map_pts, locz["row_point"],
                                  locz["row_inlier"], s["intrinsics"])
    poses = _dev(s["poses"])
    poses[loc.SCENE_MAP:] = locz["poses"][loc.SCENE_MAP:]
    PC = n_map_pts + N // 2
    xyz = torch.zeros((PC, 3), dtype=torch.float64, device="cuda")
    xyz[:n_map_pts] = tri["point_xyz"]
    tri2 = estimator.triangulate_tracks(ctx, poses, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], PC, point_select=ext["point_new"],
                                        point_xyz=xyz)
    # the extended map serves the next localisation: a new frame matched against another NEW frame
    pair = (_dev(np.array([F - 1], np.int32)), _dev(np.array([F - 2], np.int32)))
    idx1_nn = _dev(s["ext_idx1"][(s["ext_q"] == F - 2) & (s["ext_t"] == F - 1)])  # (exact pairs have q < t: read it from the other side)
    inv = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
    rows = torch.nonzero(idx1_nn[0] >= 0).flatten()
    inv[0, idx1_nn[0, rows].long()] = rows.int()
    before = estimator.gather_map_matches(ctx, kps, counts, *pair, inv, None, link["node_point"], tri["point_xyz"], None, s["intrinsics"])
    after = estimator.gather_map_matches(ctx, kps, counts, *pair, inv, None, ext["node_point"], tri2["point_xyz"], None, s["intrinsics"])
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()

    node_in, node_out = host(link["node_point"]).reshape(F, cap), host(ext["node_point"]).reshape(F, cap)
    row_point, row_inlier = host(locz["row_point"]).reshape(F, cap), host(locz["row_inlier"]).reshape(F, cap)
    totals = host(ext["totals"]).tolist()
    n_obs, n_total = totals[:2]
    truth, planted = s["true_point"], s["planted"]
    adopted = (node_out >= 0) & (node_out < n_map_pts) & (node_in < 0)
    assert adopted.sum() == totals[2] >= 3 * 60 and not adopted[:loc.SCENE_MAP].any()
    assert not (adopted & planted).any()                                           # no planted row is ADOPTED
    true_of_id = {}
    for f, i in zip(*np.nonzero(node_in >= 0)):
        assert true_of_id.setdefault(int(node_in[f, i]), int(truth[f, i])) == truth[f, i]
    assert all(true_of_id[int(node_out[f, i])] == truth[f, i] for f, i in zip(*np.nonzero(adopted)))  # ... the row's true point
    new_ids = sorted(set(node_out[node_out >= n_map_pts].tolist()))
    assert new_ids == list(range(n_map_pts, n_total)) and (len(new_ids) >= 20 if late_points else new_ids == [])
    map_obs = np.bincount(truth[:loc.SCENE_MAP][node_in[:loc.SCENE_MAP] >= 0], minlength=150)
    assert (map_obs[s["late"]] == 0).all() and (map_obs[~s["late"]] >= 2).all()
    for p in new_ids:
        behind = set(truth[node_out == p].tolist())
        assert len(behind) == 1 and -1 not in behind, p                             # one true point per new track ...
        assert map_obs[behind.pop()] < 2, p                                         # ... which had fewer than two map observations
    xyz2 = host(tri2["point_xyz"])
    assert xyz2[:n_map_pts].tobytes() == host(tri["point_xyz"]).tobytes()           # old points keep their coordinates bit for bit
    status2 = host(tri2["status"])
    assert (status2[:n_map_pts] == estimator.TRACK_SKIPPED).all() and (status2[n_total:] == estimator.TRACK_SKIPPED).all()
    n_before, n_after = int(host(before["totals"])[0]), int(host(after["totals"])[0])
    print("correspondences of frame %d against frame %d: %d through the old map, %d through the extended one" % (F - 1, F - 2, n_before, n_after))
    assert n_before == 0 and n_after > 0                                            # the unextended map holds nothing in a new frame

    # every stage against its restatement
    c_map = dict(name="scene_map", n_frames=F, cap=cap, kps=s["kps"], counts=s["counts"], pair_q=s["map_q"], pair_t=s["map_t"],
                 idx1=s["map_idx1"], inlier=np.ones_like(s["map_idx1"], np.uint8), min_views=2)
    e_link = lc.as_arrays(lc.lr.link(s["kps"][..., :2], s["counts"].tolist(), F, cap, s["map_q"].tolist(), s["map_t"].tolist(),
                                     s["map_idx1"].reshape(-1).tolist(), None, s["intrinsics"], 2), N)
    for k in LINK_OUT:
        assert host(link[k]).tobytes() == e_link[k].tobytes(), (c_map["name"], k)
    e_tri = tr.tracks(s["poses"].tolist(), e_link["obs_cam"].tolist(), e_link["obs_point"].tolist(), e_link["obs_xy"].tolist(), n_map_pts)
    assert host(tri["point_xyz"]).tobytes() == np.array(e_tri["point_xyz"], np.float64).tobytes()
    assert host(tri["status"]).tolist() == e_tri["status"]
    c_ext = dict(name="scene_extend", n_frames=F, cap=cap, kps=s["kps"], counts=s["counts"], pair_q=s["ext_q"], pair_t=s["ext_t"],
                 idx1=s["ext_idx1"], inlier=np.ones_like(s["ext_idx1"], np.uint8), node_point=node_in.reshape(-1), n_points=n_map_pts,
                 row_point=row_point.reshape(-1), row_inlier=row_inlier.reshape(-1), min_views=2)
    e_ext = ec.restate(c_ext, use_inlier=False, intrinsics=s["intrinsics"])
    got = {k: host(ext[k]) for k in OUTPUTS}
    _assert_same(got, e_ext, c_ext)
    want_ext = ec.as_arrays(e_ext, N, PC)
    e_tri2 = tr.tracks(host(poses).tolist(), want_ext["obs_cam"].tolist(), want_ext["obs_point"].tolist(), want_ext["obs_xy"].tolist(), PC,
                       point_select=want_ext["point_new"].tolist(), point_xyz=e_tri["point_xyz"] + [[0.0] * 3] * (N // 2))
    assert xyz2.tobytes() == np.array(e_tri2["point_xyz"], np.float64).tobytes()
    assert status2.tolist() == e_tri2["status"] and host(tri2["n_good"]).tolist() == e_tri2["n_good"]
    assert host(tri2["obs_good"]).tolist() == e_tri2["obs_good"]

    ok = np.flatnonzero(status2 == estimator.TRACK_OK)
    first_node = {int(p): int(np.flatnonzero(node_out.reshape(-1) == p)[0]) for p in ok}
    err = [float(np.linalg.norm(xyz2[p] - s["point_xyz_gt"][truth.reshape(-1)[n]])) for p, n in first_node.items()]
    print("totals %s; new points %d, of them OK %d; distance of the new OK points from the truth: median %.3e, largest %.3e" %
          (totals, n_total - n_map_pts, len(ok), float(np.median(err)) if err else 0.0, max(err) if err else 0.0))
