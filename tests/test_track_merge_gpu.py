"""GPU parity of gh_merge_points_dev with the plain-Python restatement tests/track_merge_restate.py, byte for byte, on the inputs
of tests/track_merge_cases.py (tests/test_track_merge_cpu.py shows what they reach): the census and the boundary soups in all
sixteen variants, the pair a fused multiply-add would decide the other way, the hub, the chain and the random split map in
three pair orders; in place against out of place; the argument contract; the device against gh_link_tracks_dev where the
contract says they agree; then the call in its place: gather on a split map -> merge -> triangulate the survivors -> gather,
without a read-back in between.  Every output buffer goes in with every byte 0xA5 and 16 bytes longer than its capacity, so
that an entry left out and a write past the end both show."""
import ctypes as C
import itertools

import numpy as np
import pytest

import localize_cases as loc
import track_link_cases as lc
import track_merge_cases as mc
import track_merge_restate as mr

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
OUTPUTS, DTYPE = mc.OUTPUTS, mc.DTYPE
TAIL = 16
FILL = loc.FILL
SCENE_MAX_DIST = 1e-3  # world units; the scene is a few units across and its pixels are exact up to float32 rounding
VARIANTS = list(itertools.product((True, False), (True, False), (True, False), (1, 0)))  # inlier, status, gate, bridge


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(N, n_points):
    return dict(point_remap=4 * n_points, point_state=n_points, point_select=n_points, node_point=4 * N, obs_point=4 * N,
                point_len=4 * n_points, totals=24)


def _dirty(N, n_points):
    import torch
    return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in _bytes(N, n_points).items()}


def _untouched(out, but=()):
    return all((t == FILL).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_inlier=True, use_status=True, use_gate=True, use_obs=True):
    d = {k: _dev(c[k]) for k in ("counts", "pair_q", "pair_t", "idx1", "node_point")}
    d["inlier"] = _dev(c["inlier"]) if use_inlier else None
    d["status"] = _dev(c["status"]) if use_status else None
    d["xyz"] = _dev(c["xyz"]) if use_gate else None
    d["obs_point"] = _dev(c["obs_point"]) if use_obs else None
    for k in ("pair_q", "pair_t", "idx1"):  # (an empty tensor has no storage)
        if d[k].numel() == 0:
            d[k] = None
    return d


def _call(ctx_h, d, out, sizes, max_dist, bridge):
    from gslam_amd import hip
    F, cap, P, n_points = sizes
    return hip.lib.gh_merge_points_dev(ctx_h, _ptr(d["counts"]), F, cap, _ptr(d["pair_q"]), _ptr(d["pair_t"]), P, _ptr(d["idx1"]),
                                       _ptr(d["inlier"]), _ptr(d["node_point"]), n_points, _ptr(d["status"]), _ptr(d["xyz"]),
                                       C.c_double(max_dist), bridge, _ptr(d["obs_point"]), *(_ptr(out[k]) for k in OUTPUTS))


def _sizes(c):
    return c["n_frames"], c["cap"], len(c["pair_q"]), c["n_points"]


def _host(out, N, n_points):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k, n in _bytes(N, n_points).items():
        if out[k] is None:
            got[k] = None
            continue
        raw = out[k].cpu().numpy()
        assert (raw[n:] == FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(DTYPE[k])
    return got


def _run(ctx, c, use_inlier=True, use_status=True, use_gate=True, bridge=1, use_obs=True):
    """gh_merge_points_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    N = c["n_frames"] * c["cap"]
    out = _dirty(N, c["n_points"])
    if not use_obs:
        out["obs_point"] = None
    st = _call(ctx.h, _inputs(c, use_inlier, use_status, use_gate, use_obs), out, _sizes(c), c["max_dist"], bridge)
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return _host(out, N, c["n_points"])


def _assert_same(got, e, c, note=()):
    want = mc.as_arrays(e)
    assert got["totals"].tolist() == want["totals"].tolist(), (c["name"], note, got["totals"], want["totals"])
    for k in OUTPUTS:
        if want[k] is None:
            assert got[k] is None
            continue
        assert got[k].dtype == want[k].dtype and got[k].tolist() == want[k].tolist(), (c["name"], note, k)
        assert got[k].tobytes() == want[k].tobytes(), (c["name"], note, k)


@pytest.mark.parametrize("use_inlier,use_status,use_gate,bridge", VARIANTS)
def test_census_matches_the_restatement_byte_for_byte(ctx, use_inlier, use_status, use_gate, bridge):
    c = mc.census()
    _assert_same(_run(ctx, c, use_inlier, use_status, use_gate, bridge), mc.restate(c, use_inlier, use_status, use_gate, bridge), c)


@pytest.mark.parametrize("which", [0, 1])
def test_block_boundaries(ctx, which):
    c = mc.boundaries()[which]
    assert (c["n_frames"] * c["cap"], c["n_points"]) == ((512, 257), (513, 256))[which]
    for v in VARIANTS:
        _assert_same(_run(ctx, c, *v), mc.restate(c, *v), c, v)
    _assert_same(_run(ctx, c, use_obs=False), mc.restate(c, use_obs=False), c, "no observation list")


def test_the_gate_is_not_fused(ctx):
    """The verdict a fused dx * dx + dy * dy would give on this pair is the other one (tests/test_track_merge_cpu.py)."""
    c = mc.fused()
    _assert_same(_run(ctx, c), mc.restate(c), c)


def _orders(ctx, c, e, seed):
    first = None
    for order in ("forward", "reversed", "shuffled"):
        for _ in range(2):
            got = _run(ctx, mc.reorder(c, order, seed=seed))
            _assert_same(got, e, c, order)
            first = first or got
            assert all(got[k].tobytes() == first[k].tobytes() for k in OUTPUTS), order


@pytest.mark.parametrize("conflict", [False, True])
def test_257_points_on_one_root(ctx, conflict):
    c = mc.hub(conflict)
    e = mc.restate(c)
    assert e["totals"] == ([0, 0, 1, 0, 0, 257] if conflict else [1, 256, 0, 0, 256, 0])
    _orders(ctx, c, e, 3)


def test_chain_of_300_points_in_any_pair_order_gives_the_same_bytes(ctx):
    c = mc.chain()
    e = mc.restate(c)
    assert e["totals"] == [1, 299, 0, 0, 598, 0]
    _orders(ctx, c, e, 3)


def test_random_split_map_in_any_pair_order_gives_the_same_bytes(ctx):
    c, e = mc.random_case()
    assert e["totals"][0] >= 10 and e["totals"][2] >= 2 and e["totals"][3] >= 2
    _orders(ctx, c, e, 4)
    for v in ((False, True, True, 1), (True, True, False, 1), (True, True, True, 0)):
        _assert_same(_run(ctx, c, *v), mc.restate(c, *v), c, v)


def test_in_place_equals_out_of_place(ctx):
    import torch
    from gslam_amd import estimator
    for c in (mc.census(), mc.random_case()[0], mc.boundaries()[1]):
        d = _inputs(c)
        args = (ctx, d["counts"], c["cap"], d["pair_q"], d["pair_t"], d["idx1"], d["inlier"])
        kw = dict(point_status=d["status"], point_xyz=d["xyz"], max_dist=c["max_dist"])
        apart = estimator.merge_points(*args, d["node_point"], c["n_points"], obs_point=d["obs_point"], **kw)
        node, obs = d["node_point"].clone(), d["obs_point"].clone()
        inpl = estimator.merge_points(*args, node, c["n_points"], obs_point=obs, in_place=True, **kw)
        torch.cuda.synchronize()
        assert inpl["node_point"].data_ptr() == node.data_ptr() and inpl["obs_point"].data_ptr() == obs.data_ptr()
        assert list(apart) == list(inpl) == list(OUTPUTS)
        assert (d["node_point"].cpu().numpy() == c["node_point"]).all()  # out of place leaves its input alone
        e = mc.as_arrays(mc.restate(c))
        for k in OUTPUTS:
            assert apart[k].cpu().numpy().tobytes() == inpl[k].cpu().numpy().tobytes() == e[k].tobytes(), (c["name"], k)


def test_argument_errors_leave_the_outputs_alone(ctx):
    c = mc.census()
    F, cap, P, n_points = _sizes(c)
    d = _inputs(c)
    out = _dirty(F * cap, n_points)
    nan = float("nan")

    def call(ctx_h=ctx.h, sizes=(F, cap, P, n_points), max_dist=c["max_dist"], null=()):
        dd = {k: (None if k in null else t) for k, t in d.items()}
        oo = {k: (None if "out_" + k in null else t) for k, t in out.items()}
        return _call(ctx_h, dd, oo, sizes, max_dist, 1)

    assert call(ctx_h=None) == GH_ERR_ARG
    for sizes in ((-1, cap, P, n_points), (F, -1, P, n_points), (F, cap, -1, n_points), (F, cap, P, -1), (1, 65536, P, n_points),
                  (32769, 65535, P, n_points), (2**31 - 1, 1, P, n_points), (F, cap, P, 2**31 - 1 - F * cap),
                  (F, cap, P, 2**31 - 1), (32768, 65535, P, 2**31 - 1 - 32768 * 65535)):
        assert call(sizes=sizes) == GH_ERR_ARG, sizes
    for bad in (-1.0, -1e-300, nan, -float("inf")):
        assert call(max_dist=bad) == GH_ERR_ARG, bad
    for k in ("counts", "pair_q", "pair_t", "idx1", "node_point", "obs_point") + tuple("out_" + k for k in OUTPUTS):
        assert call(null=(k,)) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: no inlier bytes, no status, no gate (then max_dist is not looked at), no observation list
    for null, max_dist in ((("inlier",), 5.0), (("status",), 5.0), (("xyz",), nan), (("xyz",), -1.0), (("obs_point", "out_obs_point"), 5.0)):
        assert call(null=null, max_dist=max_dist) == 0, null
    ctx.sync()
    assert not any((t[:-TAIL] == FILL).all().item() for t in out.values()) and all((t[-TAIL:] == FILL).all().item() for t in out.values())


def test_degenerate_sizes(ctx):
    import torch
    c = mc.census()
    d = _inputs(c)
    F, cap, P, n_points = _sizes(c)
    for f, k in ((0, cap), (F, 0), (0, 0)):  # N == 0: the point arrays and the totals
        out = _dirty(F * cap, n_points)
        assert _call(ctx.h, d, out, (f, k, P, n_points), c["max_dist"], 1) == 0
        torch.cuda.synchronize()
        assert _untouched(out, but=("point_remap", "point_state", "point_select", "point_len", "totals"))
        got = _host(out, 0, n_points)
        assert got["point_remap"].tolist() == list(range(n_points)) and not got["point_state"].any() and not got["point_select"].any()
        assert not got["point_len"].any() and got["totals"].tolist() == [0] * 6
    out = _dirty(F * cap, n_points)  # N == 0 and n_points == 0: the totals only
    assert _call(ctx.h, d, out, (0, cap, P, 0), c["max_dist"], 1) == 0
    torch.cuda.synchronize()
    assert _untouched(out, but=("totals",)) and _host(out, 0, 0)["totals"].tolist() == [0] * 6
    # no pairs: nothing merges, node_point and obs_point are copied, point_len is counted; the pair arrays may be NULL then
    e = dict(c, pair_q=c["pair_q"][:0], pair_t=c["pair_t"][:0], idx1=c["idx1"][:0], inlier=c["inlier"][:0], name="no_pairs")
    got = _run(ctx, e, use_inlier=False)
    _assert_same(got, mc.restate(e, False), e)
    assert got["totals"].tolist() == [0] * 6 and got["node_point"].tolist() == c["node_point"].tolist()
    assert got["point_len"].sum() == (c["obs_point"] >= 0).sum() and got["point_len"][1] == 1
    # no points: every value of node_point is "no id" and is copied
    e = dict(c, n_points=0, status=c["status"][:0], xyz=c["xyz"][:0], obs_point=np.full(F * cap, -1, np.int32), name="no_points")
    got = _run(ctx, e)
    _assert_same(got, mc.restate(e), e)
    assert got["node_point"].tolist() == c["node_point"].tolist()


def _link(ctx, c, use_inlier):
    """gh_link_tracks_dev, min_views = 2 -> (node_point, totals) as host arrays."""
    import torch
    from gslam_amd import estimator
    out = estimator.link_tracks(ctx, _dev(c["kps"]), _dev(c["counts"]), _dev(c["pair_q"]), _dev(c["pair_t"]), _dev(c["idx1"]),
                                _dev(c["inlier"]) if use_inlier else None, lc.INTRINSICS, 2)
    torch.cuda.synchronize()
    return out["node_point"].cpu().numpy(), out["totals"].cpu().numpy()


def test_every_node_its_own_point_equals_gh_link_tracks_dev(ctx):
    """The device against the device: no restatement takes part.  n_points = N, node n holds point n, no gate: the MERGED groups
    are the link's tracks and the CONFLICT groups its CONFLICT components, the labels the smallest nodes."""
    for c in lc.census() + [lc.random_case()[0], lc.chain("shuffled", seed=3), lc.hub(), lc.hub(True)]:
        N = c["n_frames"] * c["cap"]
        own = dict(c, node_point=np.arange(N, dtype=np.int32), n_points=N, status=np.zeros(N, np.int32), xyz=np.zeros((N, 3)),
                   max_dist=0.0, obs_point=np.full(N, -1, np.int32))
        for use_inlier in (True, False):
            node_point, totals = _link(ctx, c, use_inlier)
            got = _run(ctx, own, use_inlier, False, False, 1)
            assert got["totals"][[0, 2]].tolist() == totals[1:3].tolist(), (c["name"], use_inlier)
            first = {}  # link id -> its smallest node
            for n in np.flatnonzero(node_point >= 0):
                first.setdefault(int(node_point[n]), int(n))
            want_remap = np.arange(N)
            track = node_point >= 0
            want_remap[track] = [first[int(p)] for p in node_point[track]]
            assert got["point_remap"].tolist() == want_remap.tolist(), (c["name"], use_inlier)
            conflict = node_point == lc.lr.CONFLICT
            assert ((got["point_state"] == mr.CONFLICT) == conflict).all(), (c["name"], use_inlier)
            assert ((got["point_state"] == mr.SURVIVOR) | (got["point_state"] == mr.ABSORBED))[track].all()
            assert not got["point_state"][~track & ~conflict].any()


def test_a_split_map_heals_without_a_read_back(ctx):
    """mc.scene_split(): gather the new frames' matches through the split map (the rows that see both halves of a split point
    are AMBIGUOUS) -> merge with the map pairs -> triangulate the survivors from all of their observations -> gather again.
    Nothing is read back before the last call has been issued.  node_point, and row_point, offsets and totals of the second
    gather, equal byte for byte what the unsplit map gives.  The distance of the survivors from the truth is printed, not
    asserted: there is no reference value for it."""
    import torch
    from gslam_amd import estimator
    import track_extend_cases as ec
    s = mc.scene_split()
    F, cap, P = s["n_frames"], s["cap"], s["n_points"]
    kps, counts, poses = _dev(s["kps"]), _dev(s["counts"]), _dev(s["poses"])
    new = (_dev(s["new_q"]), _dev(s["new_t"]), _dev(s["new_idx1"]), None)
    obs_cam, obs_xy = _dev(s["obs_cam"]), _dev(s["obs_xy"])

    tri0 = estimator.triangulate_tracks(ctx, poses, obs_cam, _dev(s["obs_point"]), obs_xy, P)            # the unsplit map
    want = estimator.gather_map_matches(ctx, kps, counts, *new, _dev(s["node_point"]), tri0["point_xyz"], tri0["status"], s["intrinsics"])
    node_point, obs_point = _dev(s["node_point_split"]), _dev(s["obs_point_split"])                      # the split map
    tri1 = estimator.triangulate_tracks(ctx, poses, obs_cam, obs_point, obs_xy, P)
    before = estimator.gather_map_matches(ctx, kps, counts, *new, node_point, tri1["point_xyz"], tri1["status"], s["intrinsics"])
    status1, xyz1 = tri1["status"].clone(), tri1["point_xyz"].clone()
    # the status and the coordinates of the split map's own triangulation: every half has at least two views of a noise-free scene
    m = estimator.merge_points(ctx, counts, cap, _dev(s["map_q"]), _dev(s["map_t"]), _dev(s["map_idx1"]), None, node_point, P,
                               point_status=status1, point_xyz=xyz1, max_dist=SCENE_MAX_DIST, obs_point=obs_point, in_place=True)
    tri2 = estimator.triangulate_tracks(ctx, poses, obs_cam, m["obs_point"], obs_xy, P, point_select=m["point_select"], point_xyz=xyz1)
    status2 = torch.where(m["point_select"] != 0, tri2["status"], status1)  # (that call marks what it skips SKIPPED: keep the map's)
    after = estimator.gather_map_matches(ctx, kps, counts, *new, m["node_point"], tri2["point_xyz"], status2, s["intrinsics"])
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()

    k = len(s["split"])
    assert host(m["totals"]).tolist() == [k, k, 0, 0, int((s["node_point_split"] != s["node_point"]).sum()), 0]
    assert host(m["node_point"]).tobytes() == s["node_point"].tobytes() and host(m["obs_point"]).tobytes() == s["obs_point"].tobytes()
    survivors = np.flatnonzero(host(m["point_select"]))
    assert sorted(survivors.tolist()) == sorted(s["split"].values())
    assert (host(tri2["status"])[survivors] == estimator.TRACK_OK).all()                                  # every survivor triangulates
    # the split map made the rows that see both halves AMBIGUOUS; they are rows of the split points
    row_before, row_want = host(before["row_point"]), host(want["row_point"])
    ambiguous = np.flatnonzero(row_before == estimator.LOC_AMBIGUOUS)
    assert host(before["totals"])[1] == len(ambiguous) > 0 and host(want["totals"])[1] == 0
    assert set(row_want[ambiguous].tolist()) <= set(s["split"].values())
    for key in ("row_point", "offsets", "totals"):
        assert host(after[key]).tobytes() == host(want[key]).tobytes(), key
    truth = ec.scene()["true_point"].reshape(-1)
    gt = ec.scene()["point_xyz_gt"]
    err = [float(np.linalg.norm(host(tri2["point_xyz"])[p] - gt[truth[np.flatnonzero(s["node_point"] == p)[0]]])) for p in survivors]
    half = [float(np.linalg.norm(host(tri1["point_xyz"])[p] - gt[truth[np.flatnonzero(s["node_point"] == p)[0]]])) for p in survivors]
    print("merged %d points; %d rows were AMBIGUOUS; distance of the survivors from the truth: median %.3e, largest %.3e (as halves: "
          "median %.3e, largest %.3e)" % (k, len(ambiguous), np.median(err), max(err), np.median(half), max(half)))
