"""GPU parity of gh_pnp_gather_pairs_dev with the plain-Python restatement tests/localize_restate.py, byte for byte, on the
inputs of tests/localize_cases.py (tests/test_localize_cpu.py shows what they reach): the census (and with it the input of
tests/map_wide_cases.py, more than 1024 * 256 nodes), a hub voted on by 256 pairs,
a random map in three pair orders; the argument contract; then gh_localize_pairs_dev on a synthetic scene, held bit for bit
to the composition of the public pieces and to the planted truth.  Every output buffer goes in with every byte 0xA5 and 16
bytes longer than its capacity, so that an entry left out and a write past the end both show."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as lc
import localize_restate as lr
import map_wide_cases as wide

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
GATHER_OUT = ("row_point", "offsets", "xyz", "xy", "corr_node", "totals")
PNP_OUT = ("models", "ransac_inliers", "poses", "info", "summaries", "row_inlier")
DTYPE = dict(row_point=np.int32, offsets=np.int32, xyz=np.float64, xy=np.float64, corr_node=np.int32, totals=np.int32,
             models=np.float64, ransac_inliers=np.int32, poses=np.float64, info=np.float64, summaries=np.uint8, row_inlier=np.uint8)
TAIL = 16
# Largest deviation of a new frame's pose from the planted truth (translation, world units; quaternion entries) that the
# composition of the existing entries -- link_tracks, triangulate_tracks, the gather restated on the host, pnp_batch --
# leaves on the fixed scene of localize_cases.scene(): measured on an MI355X, frame 6 / 7 / 8: translation 2.268e-07 /
# 1.603e-07 / 1.920e-07, quaternion 8.26e-09 / 8.52e-09 / 9.87e-09 (the pixels are rounded to float32).  The bound is four
# times the largest, because the scene is fixed and the arithmetic deterministic.
MEASURED_POSE_ERROR = 2.267695e-07
POSE_BOUND = 4 * MEASURED_POSE_ERROR


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(F, cap):
    N = F * cap
    return dict(row_point=4 * N, offsets=4 * (F + 1), xyz=24 * N, xy=16 * N, corr_node=4 * N, totals=16, models=96 * F,
                ransac_inliers=4 * F, poses=56 * F, info=288 * F, summaries=64 * F, row_inlier=N)


def _dirty(F, cap, names=GATHER_OUT):
    import torch
    return {k: torch.full((_bytes(F, cap)[k] + TAIL,), lc.FILL, dtype=torch.uint8, device="cuda") for k in names}


def _untouched(out, but=()):
    return all((t == lc.FILL).all().item() for k, t in out.items() if k not in but)


def _inputs(c, use_keep=True, use_status=True):
    d = {k: _dev(c[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "node_point", "point_xyz")}
    d["keep"] = _dev(c["keep"]) if use_keep else None
    d["status"] = _dev(c["status"]) if use_status else None
    for k in ("pair_q", "pair_t", "idx1", "point_xyz"):  # (an empty tensor has no storage)
        if d[k].numel() == 0:
            d[k] = None
    return d


def _gather_args(ctx_h, d, sizes, intrinsics):
    F, cap, P, n_points = sizes
    return [ctx_h, _ptr(d["kps"]), _ptr(d["counts"]), F, cap, _ptr(d["pair_q"]), _ptr(d["pair_t"]), P, _ptr(d["idx1"]), _ptr(d["keep"]),
            _ptr(d["node_point"]), n_points, _ptr(d["point_xyz"]), _ptr(d["status"])] + [C.c_double(v) for v in intrinsics]


def _call(ctx_h, d, out, sizes, intrinsics=lc.INTRINSICS):
    from gslam_amd import hip
    return hip.lib.gh_pnp_gather_pairs_dev(*_gather_args(ctx_h, d, sizes, intrinsics), *(_ptr(out[k]) for k in GATHER_OUT))


def _call_localize(ctx_h, d, out, sizes, intrinsics=lc.INTRINSICS, ransac_threshold=0.006, min_rows=0, inlier_threshold=0.006):
    from gslam_amd import hip
    return hip.lib.gh_localize_pairs_dev(*_gather_args(ctx_h, d, sizes, intrinsics), C.c_double(ransac_threshold), C.c_uint64(1), 63, None,
                                         min_rows, C.c_double(inlier_threshold), *(_ptr(out[k]) for k in GATHER_OUT + PNP_OUT))


def _sizes(c):
    return c["n_frames"], c["cap"], len(c["pair_q"]), len(c["point_xyz"])


def _host(out, F, cap, names=GATHER_OUT):
    """The buffers as host arrays at their capacity, after checking that nothing was written past it."""
    got = {}
    for k in names:
        raw, n = out[k].cpu().numpy(), _bytes(F, cap)[k]
        assert (raw[n:] == lc.FILL).all(), (k, "written past its capacity")
        got[k] = raw[:n].copy().view(DTYPE[k])
    return got


def _run(ctx, c, use_keep=True, use_status=True):
    """gh_pnp_gather_pairs_dev on dirty output buffers -> dict of host arrays at their capacity."""
    import torch
    from gslam_amd import hip
    out = _dirty(c["n_frames"], c["cap"])
    st = _call(ctx.h, _inputs(c, use_keep, use_status), out, _sizes(c))
    assert st == 0, (c["name"], st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return _host(out, c["n_frames"], c["cap"])


def _assert_same(got, e, c):
    want = lc.as_arrays(e, c["n_frames"], c["cap"])
    assert got["totals"].tolist() == want["totals"].tolist(), (c["name"], got["totals"], want["totals"])
    assert got["row_point"].tolist() == want["row_point"].tolist(), c["name"]
    assert got["offsets"].tolist() == want["offsets"].tolist(), c["name"]
    for k in GATHER_OUT:
        assert got[k].tobytes() == want[k].tobytes(), (c["name"], k)


@pytest.mark.parametrize("use_keep,use_status", [(True, True), (False, False), (True, False)])
def test_census_matches_the_restatement_byte_for_byte(ctx, use_keep, use_status):
    for c in lc.census():  # per case first: a failure names the case
        _assert_same(_run(ctx, c, use_keep, use_status), lc.restate(c, use_keep, use_status), c)
    c = wide.localize_case()  # N + 1 > 1024 * 256: the second trip through the loop of loc_flags, with verdicts to count in it
    _assert_same(_run(ctx, c, use_keep, use_status), wide.localize_restated(use_keep, use_status), c)


def test_hub_voted_on_by_256_pairs(ctx):
    for c, e in lc.hub_cases():
        first = None
        for order in ("forward", "reversed", "shuffled"):
            got = _run(ctx, lc.reorder(c, order, seed=3))
            _assert_same(got, e, c)
            first = first or got
            assert all(got[k].tobytes() == first[k].tobytes() for k in GATHER_OUT), (c["name"], order)
        assert got["totals"].tolist() == ([1, 0, 0, 1] if c["name"] == "hub" else [0, 1, 0, 0])


@pytest.mark.parametrize("flags", [(True, True), (False, False)])
def test_random_map_in_any_pair_order_gives_the_same_bytes(ctx, flags):
    c, with_both, without = lc.random_case()
    e = with_both if flags[0] else without
    assert e["totals"][0] >= 60 and e["totals"][1] >= 1 and e["totals"][2] >= 1
    first = None
    for order in ("forward", "reversed", "shuffled"):
        got = _run(ctx, lc.reorder(c, order, seed=4), *flags)
        _assert_same(got, e, c)
        first = first or got
        for k in GATHER_OUT:
            assert got[k].tobytes() == first[k].tobytes(), (order, k)


def test_argument_errors_leave_the_outputs_alone(ctx):
    c = lc.census()[0]
    F, cap, P, n_points = _sizes(c)
    d = _inputs(c)
    out = _dirty(F, cap, GATHER_OUT + PNP_OUT)
    nan = float("nan")

    def call(ctx_h=ctx.h, sizes=(F, cap, P, n_points), intrinsics=lc.INTRINSICS, null=None, fn=_call, **kw):
        dd = {k: (None if k == null else t) for k, t in d.items()}
        oo = {k: (None if k == null else t) for k, t in out.items()}
        return fn(ctx_h, dd, oo, sizes, intrinsics, **kw)

    for fn in (_call, _call_localize):
        assert call(ctx_h=None, fn=fn) == GH_ERR_ARG
        for sizes in ((-1, cap, P, n_points), (F, -1, P, n_points), (F, cap, -1, n_points), (F, cap, P, -1), (1, 65536, P, n_points),
                      (32769, 65535, P, n_points), (2**31 - 1, 1, P, n_points)):
            assert call(sizes=sizes, fn=fn) == GH_ERR_ARG, sizes
        fx, fy, cx, cy = lc.INTRINSICS
        for bad in ((0.0, fy), (-1.0, fy), (nan, fy), (fx, 0.0), (fx, -2.0), (fx, nan)):
            assert call(intrinsics=bad + (cx, cy), fn=fn) == GH_ERR_ARG, bad
        for k in ("kps", "counts", "node_point", "point_xyz", "pair_q", "pair_t", "idx1") + GATHER_OUT:
            assert call(null=k, fn=fn) == GH_ERR_ARG, k
    # what only the composed call rejects: the scalars and the outputs of gh_pnp_batch_dev, its own output
    for kw in (dict(ransac_threshold=-1.0), dict(ransac_threshold=nan), dict(inlier_threshold=-1.0), dict(inlier_threshold=nan),
               dict(min_rows=-1)):
        assert call(fn=_call_localize, **kw) == GH_ERR_ARG, kw
    for k in ("models", "ransac_inliers", "poses", "summaries", "row_inlier"):
        assert call(null=k, fn=_call_localize) == GH_ERR_ARG, k
    ctx.sync()
    assert _untouched(out)
    # what the contract allows: no keep bytes, no status, no information matrices
    assert call(null="keep") == 0 and call(null="status") == 0
    ctx.sync()
    assert not _untouched(out, but=PNP_OUT) and _untouched(out, but=GATHER_OUT)
    assert call(null="info", fn=_call_localize) == 0
    ctx.sync()
    assert _untouched(out, but=GATHER_OUT + tuple(k for k in PNP_OUT if k != "info"))


def test_degenerate_sizes(ctx):
    import torch
    c = lc.census()[0]
    d = _inputs(c)
    F, cap, P, n_points = _sizes(c)
    for f, k in ((0, cap), (F, 0), (0, 0)):  # N == 0: only offsets and totals, zeros
        out = _dirty(F, cap)
        assert _call(ctx.h, d, out, (f, k, P, n_points)) == 0
        torch.cuda.synchronize()
        assert _untouched(out, but=("offsets", "totals"))
        assert out["totals"].cpu().numpy()[:16].view(np.int32).tolist() == [0, 0, 0, 0] and (out["totals"][16:] == lc.FILL).all().item()
        offsets = out["offsets"].cpu().numpy()
        assert not offsets[:4 * (f + 1)].any() and (offsets[4 * (f + 1):] == lc.FILL).all()
    # no pairs, no points: every existing node is NO_POINT, everything else is padding; the arrays they make empty may be NULL
    counts = np.array([8, 5, 0, -2, 11, 1], np.int32)
    no_pairs = dict(c, pair_q=c["pair_q"][:0], pair_t=c["pair_t"][:0], idx1=c["idx1"][:0], keep=c["keep"][:0], counts=counts, name="no_pairs")
    no_points = dict(c, point_xyz=c["point_xyz"][:0], status=c["status"][:0], counts=counts, name="no_points")
    for e in (no_pairs, no_points):
        got = _run(ctx, e, use_keep=False, use_status=False)
        _assert_same(got, lc.restate(e, False, False), e)
        assert got["totals"].tolist() == [0, 0, 0, 0] and (got["row_point"] == lr.NO_POINT).sum() == 8 + 5 + 8 + 1
        assert (got["corr_node"] == -1).all() and not got["xyz"].any() and not got["xy"].any() and not got["offsets"].any()


def _pose_error(poses, truth):
    """Largest deviation over the frames: translation (norm) and quaternion (norm of the difference, signs aligned)."""
    worst = 0.0
    for p, t in zip(poses, truth):
        q = p[:4] if np.dot(p[:4], t[:4]) >= 0 else -p[:4]
        worst = max(worst, float(np.linalg.norm(p[4:] - t[4:])), float(np.linalg.norm(q - t[:4])))
    return worst


def test_localize_equals_the_composition_and_finds_the_planted_poses(ctx):
    """The map from exact matches of 6 frames (link_tracks, triangulate_tracks at the true poses, padded arrays, no host read);
    3 new frames matched against every map frame, a tenth of their rows planted wrong.  localize_pairs must equal
    gather_map_matches + pnp_batch + a host scatter bit for bit, keep every planted row out of row_inlier, and put the new
    frames where they are."""
    import torch
    from gslam_amd import estimator
    s = lc.scene()
    F, cap = s["n_frames"], s["cap"]
    N = F * cap
    assert s["planted_error"] > 10 * max(lc.SCENE_RANSAC_THRESHOLD, lc.SCENE_INLIER_THRESHOLD)  # far outside the thresholds
    kps, counts = _dev(s["kps"]), _dev(s["counts"])
    link = estimator.link_tracks(ctx, kps, counts, _dev(s["map_q"]), _dev(s["map_t"]), _dev(s["map_idx1"]), None, s["intrinsics"])
    tri = estimator.triangulate_tracks(ctx, _dev(s["poses"]), link["obs_cam"], link["obs_point"], link["obs_xy"], N // 2)
    args = (kps, counts, _dev(s["new_q"]), _dev(s["new_t"]), _dev(s["new_idx1"]), None, link["node_point"], tri["point_xyz"], tri["status"],
            s["intrinsics"])
    pnp = dict(ransac_threshold=lc.SCENE_RANSAC_THRESHOLD, seed=lc.SCENE_SEED, inlier_threshold=lc.SCENE_INLIER_THRESHOLD,
               want_information=True)
    loc = estimator.localize_pairs(ctx, *args, **pnp)
    gat = estimator.gather_map_matches(ctx, *args)
    ref = estimator.pnp_batch(ctx, gat["xyz"], gat["xy"], gat["offsets"], pnp["ransac_threshold"], pnp["seed"], pnp["inlier_threshold"],
                              want_information=True)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()

    for k in GATHER_OUT:
        assert host(loc[k]).tobytes() == host(gat[k]).tobytes(), k
    for k in ("models", "ransac_inliers", "poses", "info", "summaries"):
        assert host(loc[k]).tobytes() == host(ref[k]).tobytes(), k
    n_corr = int(host(gat["totals"])[0])
    want = np.array(lr.scatter(host(gat["corr_node"]).tolist(), n_corr, host(ref["inlier"]).tolist(), N), np.uint8)
    row_inlier = host(loc["row_inlier"])
    assert row_inlier.tobytes() == want.tobytes()

    # the gather against the restatement on the scene, and what the scene is for
    c = dict(name="scene", n_frames=F, cap=cap, kps=s["kps"], counts=s["counts"], pair_q=s["new_q"], pair_t=s["new_t"],
             idx1=s["new_idx1"], keep=np.ones_like(s["new_idx1"], np.uint8), node_point=host(link["node_point"]),
             point_xyz=host(tri["point_xyz"]), status=host(tri["status"]))
    _assert_same({k: host(gat[k]).reshape(-1) for k in GATHER_OUT}, lc.restate(c, False, True, s["intrinsics"]), c)
    row_point = host(loc["row_point"]).reshape(F, cap)
    new = slice(lc.SCENE_MAP, F)
    assert (row_point[new][s["planted"][new]] >= 0).all()            # every planted row IS a correspondence ...
    assert not row_inlier.reshape(F, cap)[s["planted"]].any()        # ... and none of them is an inlier
    per_frame = np.diff(host(loc["offsets"]))
    assert (per_frame[:lc.SCENE_MAP] == 0).all() and (per_frame[new] >= 60).all() and host(loc["totals"])[3] == lc.SCENE_NEW
    summaries = host(loc["summaries"]).view(estimator.SUMMARY_DTYPE).reshape(F, 2)
    assert (summaries["termination"][:lc.SCENE_MAP] == estimator.PNP_NO_START).all()   # gh_pnp_batch_dev on an empty range
    good = (row_point[new] >= 0) & ~s["planted"][new]
    assert (row_inlier.reshape(F, cap)[new][good] == 1).all()
    err = _pose_error(host(loc["poses"])[new], s["poses"][new])
    print("pose error against the planted truth %.3e, correspondences per new frame %s, planted %s" %
          (err, per_frame[new].tolist(), s["planted"][new].sum(1).tolist()))
    assert err <= POSE_BOUND
