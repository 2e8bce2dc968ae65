"""Host-side mirror of the Estimator plugin (gslam_amd/plugin/estimator_plugin.cpp): robust model fitting with
inlier masks through gh_ransac_estimate.  Mirrors GSLAM::Estimator::findHomography / findAffine2D / findFundamental /
findAffine3D (GSLAM/core/Estimator.h:100-147).  estimate_batch / estimate_pairs are the batched, device-resident entries
(gh_ransac_batch_dev / gh_ransac_pairs_dev): torch tensors are only the device buffers, as in matcher.py.  two_view_batch /
two_view_pairs (gh_two_view_batch_dev / gh_two_view_pairs_dev) go on from an essential matrix to the relative pose and the
3-D points, batched and device-resident in the same way.  pnp_refine_batch / pnp_batch (gh_pnp_refine_batch_dev /
gh_pnp_batch_dev) refine the poses of many PnP fits in one launch, each as gh_ba_pnp would on its inliers.
triangulate_tracks (gh_triangulate_tracks_dev) gives every map point of a gh_ba_problem its start from all of its observations;
link_tracks (gh_link_tracks_dev) builds those per-point arrays from the inlier rows of the pair entries.
gather_map_matches (gh_pnp_gather_pairs_dev) reads the pair matches of new frames through that map into the arrays pnp_batch
takes; localize_pairs (gh_localize_pairs_dev) registers every frame in one call and says which keypoint rows were inliers;
extend_tracks (gh_extend_tracks_dev) adds those rows to the tracks of the map and links the other rows of the new frames into
new tracks numbered after the map's, so that the map grows batch after batch without a read-back; merge_points
(gh_merge_points_dev) renames the points that the matches show to be one to the oldest id of their group; describe_points
(gh_describe_points_dev) gives every map point its representative descriptor, mean viewing direction and distance range;
search_projection (gh_search_projection_dev) projects those points into the localized frames and adds the keypoints it finds in
a window to the claims: localize_pairs -> search_projection -> extend_tracks -> triangulate_tracks -> describe_points(point_new |
point_grew)."""
import ctypes as C

import numpy as np

from . import hip

HOMOGRAPHY, AFFINE2D, FUNDAMENTAL, AFFINE3D, ESSENTIAL, SIM3, PLANE, PNP = 0, 1, 2, 3, 4, 5, 6, 7
TWO_VIEW_OK, TWO_VIEW_NO_MODEL, TWO_VIEW_TOO_FEW, TWO_VIEW_AMBIGUOUS = 0, 1, 2, 3  # GH_TWO_VIEW_*: status per problem
PNP_NO_START, PNP_TOO_FEW = 4, 5  # GH_PNP_*: termination of a batched refinement next to gh_ba_summary's 0 .. 3
# GH_TRACK_*: status per point of triangulate_tracks
TRACK_OK, TRACK_TOO_FEW, TRACK_DEGENERATE, TRACK_INCONSISTENT, TRACK_LOW_PARALLAX, TRACK_SKIPPED = 0, 1, 2, 3, 4, 5
LINK_SHORT, LINK_CONFLICT, LINK_NO_ROW = -1, -2, -3  # GH_LINK_*: what node_point of link_tracks holds where there is no point id
EXT_REJECTED = -4  # GH_EXT_REJECTED: beside LINK_*, what node_point of extend_tracks holds at a claimant that was turned down
# GH_MERGE_*: the state byte per point of merge_points
MERGE_NONE, MERGE_SURVIVOR, MERGE_ABSORBED, MERGE_CONFLICT, MERGE_FAR = 0, 1, 2, 3, 4
PDESC_OK, PDESC_EMPTY, PDESC_NOT_OK, PDESC_SKIPPED = 0, 1, 2, 3  # GH_PDESC_*: the state byte per point of describe_points
# GH_LOC_*: what row_point of gather_map_matches / localize_pairs holds where there is no point id
LOC_NO_POINT, LOC_AMBIGUOUS, LOC_NO_ROW, LOC_SHARED = -1, -2, -3, -4
RANSAC, LMEDS, NOSAMPLE = 0, 1, 2  # GSLAM::EstimatorMethod sampling flags (Estimator.h:86-89) as gh_ransac_estimate_ex takes them


def _estimate_host(ctx, fn, model, src, dst, scalars, with_used=True):
    """One host-array call of the gh_ransac_estimate family: fn(ctx, model, src, dst, n, *scalars, model, mask, &inliers
    [, &hypotheses_used]) -> (model, mask, inliers[, hypotheses_used])."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    dst = np.ascontiguousarray(dst, dtype=np.float64)
    n = src.shape[0]
    m = np.zeros(12)
    mask = np.zeros(max(n, 1), np.uint8)
    outs = [C.c_int() for _ in range(2 if with_used else 1)]
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.check(fn(ctx.h, int(model), pv(src), pv(dst), n, *scalars, pv(m), pv(mask), *(C.byref(o) for o in outs)))
    return (m, mask[:n].copy()) + tuple(o.value for o in outs)


def estimate_ex(ctx: hip.Context, model, src, dst, threshold, sampling, confidence=1.0, seed=1):
    """gh_ransac_estimate_ex -> (model, mask, inliers, hypotheses_used)."""
    return _estimate_host(ctx, hip.lib.gh_ransac_estimate_ex, model, src, dst,
                          (C.c_double(threshold), C.c_double(confidence), C.c_uint64(seed), int(sampling)))


def estimate_conf(ctx: hip.Context, model, src, dst, threshold, confidence, seed=1):
    """gh_ransac_estimate_conf -> (model, mask, inliers, hypotheses_used)."""
    return _estimate_host(ctx, hip.lib.gh_ransac_estimate_conf, model, src, dst,
                          (C.c_double(threshold), C.c_double(confidence), C.c_uint64(seed)))


def estimate(ctx: hip.Context, model, src, dst, threshold, seed=1):
    return _estimate_host(ctx, hip.lib.gh_ransac_estimate, model, src, dst, (C.c_double(threshold), C.c_uint64(seed)),
                          with_used=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def batch_tile_rows(model):
    """gh_ransac_batch_tile_rows: correspondences the batched scoring kernel stages at a time (<= 0: unknown model)."""
    return int(hip.lib.gh_ransac_batch_tile_rows(int(model)))


def estimate_batch(ctx: hip.Context, model, src, dst, offsets, threshold, seed, thresholds=None, seeds=None):
    """gh_ransac_batch_dev.  src, dst: rows x dim float64 (cuda); offsets: nproblems + 1 int32 (cuda), problem p owns rows
    offsets[p] .. offsets[p + 1] - 1; thresholds (float64) / seeds (int64 holding the uint64 bits) per problem or None for
    the scalars.  -> (models nproblems x 12 float64, mask rows uint8, inliers nproblems int32), all on the device; nothing
    is synchronised.  Problem p equals estimate(ctx, model, src_p, dst_p, threshold_p, seed_p)."""
    import torch
    assert src.is_cuda and dst.is_cuda and src.dtype == dst.dtype == torch.float64 and src.is_contiguous() and dst.is_contiguous()
    assert offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.numel() >= 1
    assert thresholds is None or (thresholds.is_cuda and thresholds.dtype == torch.float64 and thresholds.is_contiguous())
    assert seeds is None or (seeds.is_cuda and seeds.dtype == torch.int64 and seeds.is_contiguous())
    n = offsets.numel() - 1
    assert (thresholds is None or thresholds.numel() == n) and (seeds is None or seeds.numel() == n)
    models = torch.empty((n, 12), dtype=torch.float64, device=src.device)
    mask = torch.zeros(src.shape[0], dtype=torch.uint8, device=src.device)  # (rows past offsets[n], if any, belong to nobody)
    inliers = torch.empty(n, dtype=torch.int32, device=src.device)
    ctx.check(hip.lib.gh_ransac_batch_dev(ctx.h, int(model), _p(src), _p(dst), _p(offsets), n, C.c_double(threshold), _p(thresholds),
                                          C.c_uint64(seed), _p(seeds), _p(models), _p(mask), _p(inliers)))
    return models, mask, inliers


def _pair_io(kps, counts, pair_q, pair_t, idx1, keep):
    """The inputs of the pair entries, checked, and the output tensors both have, in the order of the C arguments
    -> (P, cap, out)."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, pair_q, pair_t, idx1))
    P, cap = pair_q.shape[0], kps.shape[1]
    assert pair_t.shape[0] == P and idx1.numel() == P * cap
    assert keep is None or (keep.is_cuda and keep.dtype == torch.uint8 and keep.is_contiguous() and keep.numel() == P * cap)
    out = {"models": torch.empty((P, 12), dtype=torch.float64, device=kps.device),
           "inlier": torch.empty((P, cap), dtype=torch.uint8, device=kps.device),
           "n_corr": torch.empty(P, dtype=torch.int32, device=kps.device),
           "inliers": torch.empty(P, dtype=torch.int32, device=kps.device)}
    return P, cap, out


def estimate_pairs(ctx: hip.Context, model, kps, counts, pair_q, pair_t, idx1, keep, threshold, seed):
    """gh_ransac_pairs_dev, the call after BFMatcher.match_pairs / mask.  kps: F x cap x 7 float32 view of the KeyPoint
    records, counts: F int32, pair_q / pair_t: P int32, idx1: P x cap int32, keep: P x cap uint8 or None (all cuda).
    model: HOMOGRAPHY, AFFINE2D or FUNDAMENTAL.  -> (models P x 12, inlier P x cap uint8, n_corr P int32, inliers P int32)
    on the device; pair p equals estimate() on the rows correspondences_from_matches lists for it."""
    P, cap, out = _pair_io(kps, counts, pair_q, pair_t, idx1, keep)
    ctx.check(hip.lib.gh_ransac_pairs_dev(ctx.h, int(model), _p(kps), _p(counts), cap, _p(pair_q), _p(pair_t), P, _p(idx1), _p(keep),
                                          C.c_double(threshold), C.c_uint64(seed), *(_p(out[k]) for k in out)))
    return tuple(out.values())


def correspondences_from_matches(kps, counts, pair_q, pair_t, idx1, keep=None):
    """The gather rule of gh_ransac_pairs_dev restated in numpy (host arrays).  kps: F x cap KeyPoint records (the structured
    dtype of orb.KP_DTYPE, or F x cap x 7 float32 with x, y first); idx1 / keep: P x cap.  For each pair -> (src n x 2 float64,
    dst n x 2 float64, rows n): the query rows i < counts[pair_q[p]], ascending, with keep[p, i] (if keep is given) and
    0 <= idx1[p, i] < counts[pair_t[p]]; src = the query keypoint's (x, y), dst = the matched train keypoint's."""
    kps = np.asarray(kps)
    if kps.dtype.names:
        xy = np.stack([kps["x"], kps["y"]], axis=-1)
    else:
        xy = kps[..., :2]
    xy = xy.astype(np.float64)
    cap = xy.shape[1]
    counts = np.clip(np.asarray(counts, dtype=np.int64), 0, cap)
    idx1 = np.asarray(idx1).reshape(len(pair_q), cap)
    keep = None if keep is None else np.asarray(keep).reshape(len(pair_q), cap)
    out = []
    for p, (fq, ft) in enumerate(zip(np.asarray(pair_q).tolist(), np.asarray(pair_t).tolist())):
        rows = []
        for i in range(int(counts[fq])):
            j = int(idx1[p, i])
            if (keep is None or keep[p, i]) and 0 <= j < counts[ft]:
                rows.append(i)
        rows = np.asarray(rows, dtype=np.int64)
        out.append((xy[fq, rows].reshape(-1, 2), xy[ft, idx1[p, rows]].reshape(-1, 2), rows))
    return out


def two_view_default_params():
    """gh_two_view_default_params -> hip.TwoViewParams (min_parallax_cos, max_reproj, min_good, min_good_permille)."""
    p = hip.TwoViewParams()
    hip.lib.gh_two_view_default_params(C.byref(p))
    return p


def two_view_batch(ctx: hip.Context, E, src, dst, offsets, mask=None, params=None):
    """gh_two_view_batch_dev.  E: nproblems x e_stride float64 (cuda, e_stride >= 9: the models of estimate_batch go in as they
    are), src / dst: rows x 2 float64 normalised coordinates, offsets: nproblems + 1 int32, mask: rows uint8 or None (all rows
    take part).  -> (poses nproblems x 7 [qx qy qz qw tx ty tz] ref -> cur, points rows x 3 in the reference frame, good rows
    uint8, counts nproblems x 4 int32, n_used nproblems int32, status nproblems int32: TWO_VIEW_*), all on the device;
    nothing is synchronised."""
    import torch
    assert E.is_cuda and E.dtype == torch.float64 and E.is_contiguous() and E.dim() == 2 and E.shape[1] >= 9
    assert src.is_cuda and dst.is_cuda and src.dtype == dst.dtype == torch.float64 and src.is_contiguous() and dst.is_contiguous()
    assert offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.numel() == E.shape[0] + 1
    rows = src.shape[0]
    assert mask is None or (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == rows)
    n = E.shape[0]
    prm = params if params is not None else two_view_default_params()
    dev = src.device
    poses = torch.empty((n, 7), dtype=torch.float64, device=dev)
    points = torch.zeros((rows, 3), dtype=torch.float64, device=dev)  # (rows past offsets[n], if any, belong to nobody)
    good = torch.zeros(rows, dtype=torch.uint8, device=dev)
    counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
    n_used = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.check(hip.lib.gh_two_view_batch_dev(ctx.h, _p(E), int(E.shape[1]), _p(src), _p(dst), _p(offsets), n, _p(mask), C.byref(prm),
                                            _p(poses), _p(points), _p(good), _p(counts), _p(n_used), _p(status)))
    return poses, points, good, counts, n_used, status


def two_view_pairs(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, keep, intrinsics, threshold, seed, params=None):
    """gh_two_view_pairs_dev, the call after BFMatcher.match_pairs / mask for a calibrated camera.  kps .. keep as
    estimate_pairs takes them; intrinsics: (fx, fy, cx, cy); threshold: of the essential fit, in normalised units.
    -> dict of device tensors: models P x 12, inlier P x cap uint8, n_corr P, inliers P, poses P x 7, points P x cap x 3,
    good P x cap uint8, votes P x 4 (the four candidate counts), status P.  Pair p equals estimate_batch(ESSENTIAL) and
    two_view_batch on the normalised rows correspondences_from_matches lists for it, scattered back to query rows."""
    import torch
    P, cap, out = _pair_io(kps, counts, pair_q, pair_t, idx1, keep)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    prm = params if params is not None else two_view_default_params()
    dev = kps.device
    out.update({"poses": torch.empty((P, 7), dtype=torch.float64, device=dev),
                "points": torch.empty((P, cap, 3), dtype=torch.float64, device=dev),
                "good": torch.empty((P, cap), dtype=torch.uint8, device=dev),
                "votes": torch.empty((P, 4), dtype=torch.int32, device=dev),
                "status": torch.empty(P, dtype=torch.int32, device=dev)})
    ctx.check(hip.lib.gh_two_view_pairs_dev(ctx.h, _p(kps), _p(counts), cap, _p(pair_q), _p(pair_t), P, _p(idx1), _p(keep),
                                            C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), C.c_double(threshold),
                                            C.c_uint64(seed), C.byref(prm), *(_p(out[k]) for k in out)))
    return out


SUMMARY_DTYPE = np.dtype([("iterations", "<i4"), ("accepted", "<i4"), ("termination", "<i4"), ("n_used", "<i4"),
                          ("initial_cost", "<f8"), ("final_cost", "<f8")])  # hip.PnpBatchSummary as a numpy record


def pnp_pose_from_model(model):
    """gh_pnp_pose_from_model (host only): [R row-major | t], X_cam = R X + t -> (T_wc pose [qx qy qz qw tx ty tz], ok).
    ok False: no start, the pose is zeros."""
    m = np.ascontiguousarray(model, dtype=np.float64).reshape(12)
    pose = np.full(7, np.nan)
    ok = hip.lib.gh_pnp_pose_from_model(m.ctypes.data_as(C.c_void_p), pose.ctypes.data_as(C.c_void_p))
    return pose, bool(ok)


def _ba_options(options):
    if options is not None:
        return options
    o = hip.BaOptions()
    hip.lib.gh_ba_default_options(C.byref(o))
    return o


def _pnp_io(xyz, xy, offsets, want_information, chain=False):
    """The inputs both PnP batch entries share, checked, and their output tensors in the order of the C arguments (chain: with
    the fit's outputs in front and a summary per round) -> (nproblems, rows, out)."""
    import torch
    assert xyz.is_cuda and xy.is_cuda and xyz.dtype == xy.dtype == torch.float64 and xyz.is_contiguous() and xy.is_contiguous()
    rows = xyz.shape[0]
    assert xyz.numel() == 3 * rows and xy.numel() == 2 * rows
    assert offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.numel() >= 1
    n = offsets.numel() - 1
    dev = xyz.device
    out = {}
    if chain:
        out["models"] = torch.empty((n, 12), dtype=torch.float64, device=dev)
        out["ransac_inliers"] = torch.empty(n, dtype=torch.int32, device=dev)
    size = C.sizeof(hip.PnpBatchSummary)
    out.update({"poses": torch.empty((n, 7), dtype=torch.float64, device=dev),
                "info": torch.empty((n, 36), dtype=torch.float64, device=dev) if want_information else None,
                "summaries": torch.empty((n, 2, size) if chain else (n, size), dtype=torch.uint8, device=dev),
                "inlier": torch.zeros(rows, dtype=torch.uint8, device=dev),  # (rows no range owns belong to nobody)
                "n_inliers": torch.empty(n, dtype=torch.int32, device=dev)})
    return n, rows, out


def pnp_refine_batch(ctx: hip.Context, xyz, xy, offsets, start, mask=None, dof=63, options=None, min_rows=0,
                     inlier_threshold=-1.0, want_information=False):
    """gh_pnp_refine_batch_dev.  xyz: rows x 3, xy: rows x 2 float64 (cuda); offsets: nproblems + 1 int32; start: nproblems x 7
    (T_wc poses) or nproblems x 12 (models of estimate_batch(PNP)) float64; mask: rows uint8 or None (all rows take part);
    options: hip.BaOptions or None for the defaults.  -> dict of device tensors: poses nproblems x 7, info nproblems x 36 or
    None, summaries nproblems x 32 uint8 (view the host copy as SUMMARY_DTYPE), inlier rows uint8, n_inliers nproblems int32;
    nothing is synchronised.  A problem that is optimised equals ba.pnp on its participating rows, bit for bit."""
    import torch
    n, rows, out = _pnp_io(xyz, xy, offsets, want_information)
    assert start.is_cuda and start.dtype == torch.float64 and start.is_contiguous() and start.dim() == 2 and start.shape[0] == n
    assert start.shape[1] in (7, 12)
    assert mask is None or (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == rows)
    opt = _ba_options(options)
    ctx.check(hip.lib.gh_pnp_refine_batch_dev(ctx.h, _p(xyz), _p(xy), _p(offsets), n, rows, _p(mask), _p(start), int(start.shape[1]),
                                              int(dof), C.byref(opt), int(min_rows), C.c_double(inlier_threshold),
                                              *(_p(out[k]) for k in out)))
    return out


def pnp_batch(ctx: hip.Context, xyz, xy, offsets, ransac_threshold, seed, inlier_threshold, dof=63, options=None, min_rows=0,
              want_information=False):
    """gh_pnp_batch_dev, the call after a 3D-2D gather: estimate_batch(PNP), pnp_refine_batch on its inliers from its models,
    pnp_refine_batch again on the rows within inlier_threshold from the first round's poses.  -> dict of device tensors:
    models nproblems x 12, ransac_inliers nproblems, poses nproblems x 7, info nproblems x 36 or None, summaries
    nproblems x 2 x 32 uint8 (round 1, round 2), inlier rows uint8, n_inliers nproblems; nothing is synchronised."""
    n, rows, out = _pnp_io(xyz, xy, offsets, want_information, chain=True)
    opt = _ba_options(options)
    ctx.check(hip.lib.gh_pnp_batch_dev(ctx.h, _p(xyz), _p(xy), _p(offsets), n, rows, C.c_double(ransac_threshold), C.c_uint64(seed),
                                       int(dof), C.byref(opt), int(min_rows), C.c_double(inlier_threshold),
                                       *(_p(out[k]) for k in out)))
    return out


def track_default_params():
    """gh_track_default_params -> hip.TrackParams (min_parallax_cos, max_reproj, min_views, max_drops)."""
    p = hip.TrackParams()
    hip.lib.gh_track_default_params(C.byref(p))
    return p


def track_group_lanes():
    """gh_track_group_lanes: the number of partial sums of gh_triangulate_tracks_dev (8)."""
    return int(hip.lib.gh_track_group_lanes())


def triangulate_tracks(ctx: hip.Context, cam_pose, obs_cam, obs_point, obs_xy, n_points, obs_use=None, point_select=None,
                       params=None, point_xyz=None):
    """gh_triangulate_tracks_dev, the call between pnp_batch and a BA graph.  cam_pose: n_cams x 7 float64 T_wc, obs_cam /
    obs_point: n_obs int32, obs_xy: n_obs x 2 float64 (all cuda, laid out as in a gh_ba_problem); obs_use: n_obs uint8 or None
    (all observations), point_select: n_points uint8 or None (all points); point_xyz: n_points x 3 float64 to be updated in
    place (the points that are not selected keep their values) or None for a zeroed one.  -> dict of device tensors:
    point_xyz n_points x 3, status n_points int32 (TRACK_*), n_good n_points int32, obs_good n_obs uint8; nothing is
    synchronised."""
    import torch
    assert cam_pose.is_cuda and cam_pose.dtype == torch.float64 and cam_pose.is_contiguous() and cam_pose.numel() % 7 == 0
    assert obs_xy.is_cuda and obs_xy.dtype == torch.float64 and obs_xy.is_contiguous()
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (obs_cam, obs_point))
    n_cams, n_obs, n_points = cam_pose.numel() // 7, obs_cam.numel(), int(n_points)
    assert obs_point.numel() == n_obs and obs_xy.numel() == 2 * n_obs and n_points >= 0
    assert obs_use is None or (obs_use.is_cuda and obs_use.dtype == torch.uint8 and obs_use.is_contiguous() and obs_use.numel() == n_obs)
    assert point_select is None or (point_select.is_cuda and point_select.dtype == torch.uint8 and point_select.is_contiguous() and
                                    point_select.numel() == n_points)
    dev = cam_pose.device
    if point_xyz is None:
        point_xyz = torch.zeros((n_points, 3), dtype=torch.float64, device=dev)
    assert point_xyz.is_cuda and point_xyz.dtype == torch.float64 and point_xyz.is_contiguous() and point_xyz.numel() == 3 * n_points
    prm = params if params is not None else track_default_params()
    out = {"point_xyz": point_xyz,
           "status": torch.empty(n_points, dtype=torch.int32, device=dev),
           "n_good": torch.empty(n_points, dtype=torch.int32, device=dev),
           "obs_good": torch.empty(n_obs, dtype=torch.uint8, device=dev)}
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    ctx.check(hip.lib.gh_triangulate_tracks_dev(ctx.h, p(cam_pose), n_cams, p(obs_cam), p(obs_point), p(obs_xy), n_obs, n_points,
                                                _p(obs_use), _p(point_select), C.byref(prm), *(p(out[k]) for k in out)))
    return out


def link_tracks(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, inlier, intrinsics, min_views=2):
    """gh_link_tracks_dev, the call between the pair entries and triangulate_tracks.  kps: F x cap x 7 float32 view of the
    KeyPoint records, counts: F int32, pair_q / pair_t: P int32, idx1: P x cap int32, inlier: P x cap uint8 or None (all rows):
    keep of BFMatcher.mask, inlier of estimate_pairs, inlier / good of two_view_pairs (all cuda); intrinsics: (fx, fy, cx, cy).
    With N = F * cap -> dict of device tensors: node_point N int32 (a point id, LINK_SHORT, LINK_CONFLICT or LINK_NO_ROW),
    obs_cam / obs_point / obs_node N int32 and obs_xy N x 2 float64 (padded past n_obs with -1 and zeros), point_len N // 2
    int32, totals 4 int32 (n_obs, n_points, CONFLICT components, SHORT components of two nodes or more); nothing is
    synchronised and nothing is read back: obs_cam, obs_point, obs_xy go to triangulate_tracks as they are, with
    n_points = N // 2."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, pair_q, pair_t, idx1))
    F, cap, P = kps.shape[0], kps.shape[1], pair_q.shape[0]
    assert counts.numel() == F and pair_t.shape[0] == P and idx1.numel() == P * cap
    assert inlier is None or (inlier.is_cuda and inlier.dtype == torch.uint8 and inlier.is_contiguous() and inlier.numel() == P * cap)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    N, dev = F * cap, kps.device
    out = {"node_point": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_cam": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_point": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_xy": torch.empty((N, 2), dtype=torch.float64, device=dev),
           "obs_node": torch.empty(N, dtype=torch.int32, device=dev),
           "point_len": torch.empty(N // 2, dtype=torch.int32, device=dev),
           "totals": torch.empty(4, dtype=torch.int32, device=dev)}
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    ctx.check(hip.lib.gh_link_tracks_dev(ctx.h, p(kps), p(counts), F, cap, p(pair_q), p(pair_t), P, p(idx1), _p(inlier),
                                         C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), int(min_views),
                                         *(p(out[k]) for k in out)))
    return out


def _gather_io(kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status):
    """The inputs of the two map entries, checked, and the gather's output tensors in the order of the C arguments
    -> (F, cap, P, n_points, out)."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, pair_q, pair_t, idx1, node_point))
    F, cap, P = kps.shape[0], kps.shape[1], pair_q.shape[0]
    N, dev = F * cap, kps.device
    assert counts.numel() == F and pair_t.shape[0] == P and idx1.numel() == P * cap and node_point.numel() == N
    assert keep is None or (keep.is_cuda and keep.dtype == torch.uint8 and keep.is_contiguous() and keep.numel() == P * cap)
    assert point_xyz.is_cuda and point_xyz.dtype == torch.float64 and point_xyz.is_contiguous() and point_xyz.numel() % 3 == 0
    n_points = point_xyz.numel() // 3
    assert point_status is None or (point_status.is_cuda and point_status.dtype == torch.int32 and point_status.is_contiguous() and
                                    point_status.numel() == n_points)
    out = {"row_point": torch.empty(N, dtype=torch.int32, device=dev),
           "offsets": torch.empty(F + 1, dtype=torch.int32, device=dev),
           "xyz": torch.empty((N, 3), dtype=torch.float64, device=dev),
           "xy": torch.empty((N, 2), dtype=torch.float64, device=dev),
           "corr_node": torch.empty(N, dtype=torch.int32, device=dev),
           "totals": torch.empty(4, dtype=torch.int32, device=dev)}
    return F, cap, P, n_points, out


def gather_map_matches(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status, intrinsics):
    """gh_pnp_gather_pairs_dev, the call between a map (link_tracks, triangulate_tracks) and pnp_batch.  kps: F x cap x 7 float32
    view of the KeyPoint records, counts: F int32, pair_q / pair_t: P int32 (new frame, map frame), idx1: P x cap int32, keep:
    P x cap uint8 or None (all rows); node_point: F * cap int32 as link_tracks returns it, point_xyz: n_points x 3 float64,
    point_status: n_points int32 (only TRACK_OK points are used) or None (all points) -- all cuda; intrinsics: (fx, fy, cx, cy).
    With N = F * cap -> dict of device tensors: row_point N int32 (a point id, LOC_NO_POINT, LOC_AMBIGUOUS, LOC_NO_ROW or
    LOC_SHARED), offsets F + 1 int32, xyz N x 3 and xy N x 2 float64 (zeros past n_corr), corr_node N int32 (-1 past n_corr),
    totals 4 int32 (n_corr, AMBIGUOUS nodes, SHARED nodes, frames with a correspondence); nothing is synchronised and nothing is
    read back: xyz, xy, offsets go to pnp_batch as they are."""
    F, cap, P, n_points, out = _gather_io(kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    ctx.check(hip.lib.gh_pnp_gather_pairs_dev(ctx.h, p(kps), p(counts), F, cap, p(pair_q), p(pair_t), P, p(idx1), _p(keep),
                                              p(node_point), n_points, p(point_xyz), _p(point_status), C.c_double(fx),
                                              C.c_double(fy), C.c_double(cx), C.c_double(cy), *(p(out[k]) for k in out)))
    return out


def localize_pairs(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status, intrinsics,
                   ransac_threshold, seed, inlier_threshold, dof=63, options=None, min_rows=0, want_information=False):
    """gh_localize_pairs_dev: every frame registered against the map in one call -- gather_map_matches, pnp_batch on its arrays
    (one problem per frame), and the inlier bytes of the last round scattered back to keypoint rows.  Inputs as
    gather_map_matches and pnp_batch take them.  -> dict of device tensors: the gather's (row_point, offsets, xyz, xy, corr_node,
    totals), then models F x 12, ransac_inliers F, poses F x 7, info F x 36 or None, summaries F x 2 x 32 uint8 (view the host
    copy as SUMMARY_DTYPE), row_inlier F * cap uint8 (1 where the row's correspondence is an inlier of the last round); nothing
    is synchronised.  row_point and row_inlier are what extends the tracks with the new observations."""
    import torch
    F, cap, P, n_points, out = _gather_io(kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    dev = kps.device
    out.update({"models": torch.empty((F, 12), dtype=torch.float64, device=dev),
                "ransac_inliers": torch.empty(F, dtype=torch.int32, device=dev),
                "poses": torch.empty((F, 7), dtype=torch.float64, device=dev),
                "info": torch.empty((F, 36), dtype=torch.float64, device=dev) if want_information else None,
                "summaries": torch.empty((F, 2, C.sizeof(hip.PnpBatchSummary)), dtype=torch.uint8, device=dev),
                "row_inlier": torch.empty(F * cap, dtype=torch.uint8, device=dev)})
    opt = _ba_options(options)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() or 256)
    ctx.check(hip.lib.gh_localize_pairs_dev(ctx.h, p(kps), p(counts), F, cap, p(pair_q), p(pair_t), P, p(idx1), _p(keep),
                                            p(node_point), n_points, p(point_xyz), _p(point_status), C.c_double(fx), C.c_double(fy),
                                            C.c_double(cx), C.c_double(cy), C.c_double(ransac_threshold), C.c_uint64(seed), int(dof),
                                            C.byref(opt), int(min_rows), C.c_double(inlier_threshold), *(p(out[k]) for k in out)))
    return out


def extend_tracks(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, inlier, node_point, n_points, row_point, row_inlier, intrinsics,
                  min_views=2):
    """gh_extend_tracks_dev, the call after localize_pairs: the map grows by the new frames.  kps, counts, pair_q, pair_t, idx1,
    inlier, intrinsics, min_views as link_tracks takes them; node_point: F * cap int32 as link_tracks or an earlier extend_tracks
    returned it, or None (no map); n_points: the number of map points; row_point F * cap int32 and row_inlier F * cap uint8 as
    localize_pairs returns them, or both None (no claims) -- all cuda.  With N = F * cap and PC = n_points + N // 2 -> dict of
    device tensors: node_point N int32 (a point id, LINK_SHORT, LINK_CONFLICT, EXT_REJECTED or LINK_NO_ROW), obs_cam / obs_point /
    obs_node N int32 and obs_xy N x 2 float64 (padded past n_obs with -1 and zeros), point_len PC int32, point_new PC uint8 (1 at
    the points this call created), point_grew PC uint8 (1 at the old points that got an observation), totals 6 int32 (n_obs,
    n_points_total, ADOPTED nodes, REJECTED nodes, CONFLICT components, SHORT components of two nodes or more); nothing is
    synchronised and nothing is read back: obs_cam, obs_point, obs_xy go to triangulate_tracks as they are, with n_points = PC
    and point_select = point_new (keep the map's status array apart: that call marks every old point TRACK_SKIPPED)."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, pair_q, pair_t, idx1))
    F, cap, P = kps.shape[0], kps.shape[1], pair_q.shape[0]
    N, dev, n_points = F * cap, kps.device, int(n_points)
    assert counts.numel() == F and pair_t.shape[0] == P and idx1.numel() == P * cap and n_points >= 0
    assert inlier is None or (inlier.is_cuda and inlier.dtype == torch.uint8 and inlier.is_contiguous() and inlier.numel() == P * cap)
    assert node_point is None or (node_point.is_cuda and node_point.dtype == torch.int32 and node_point.is_contiguous() and
                                  node_point.numel() == N)
    assert (row_point is None) == (row_inlier is None)
    assert row_point is None or (row_point.is_cuda and row_point.dtype == torch.int32 and row_point.is_contiguous() and
                                 row_point.numel() == N and row_inlier.is_cuda and row_inlier.dtype == torch.uint8 and
                                 row_inlier.is_contiguous() and row_inlier.numel() == N)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    PC = n_points + N // 2
    out = {"node_point": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_cam": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_point": torch.empty(N, dtype=torch.int32, device=dev),
           "obs_xy": torch.empty((N, 2), dtype=torch.float64, device=dev),
           "obs_node": torch.empty(N, dtype=torch.int32, device=dev),
           "point_len": torch.empty(PC, dtype=torch.int32, device=dev),
           "point_new": torch.empty(PC, dtype=torch.uint8, device=dev),
           "point_grew": torch.empty(PC, dtype=torch.uint8, device=dev),
           "totals": torch.empty(6, dtype=torch.int32, device=dev)}
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    q = lambda t: None if t is None else p(t)  # (NULL means "not given" for these three, also when N == 0)
    ctx.check(hip.lib.gh_extend_tracks_dev(ctx.h, p(kps), p(counts), F, cap, p(pair_q), p(pair_t), P, p(idx1), _p(inlier),
                                           q(node_point), n_points, q(row_point), q(row_inlier), C.c_double(fx), C.c_double(fy),
                                           C.c_double(cx), C.c_double(cy), int(min_views), *(p(out[k]) for k in out)))
    return out


def merge_points(ctx: hip.Context, counts, cap, pair_q, pair_t, idx1, inlier, node_point, n_points, point_status=None, point_xyz=None,
                 max_dist=0.0, bridge=True, obs_point=None, in_place=False):
    """gh_merge_points_dev, the call after extend_tracks: map points that the pair matches join are merged into the smallest id
    of their group.  counts: F int32, cap: the rows per frame, pair_q / pair_t: P int32, idx1: P x cap int32, inlier: P x cap
    uint8 or None (all rows), as link_tracks takes them; node_point: F * cap int32 as extend_tracks returns it; n_points: the
    capacity of the point arrays (the PC of extend_tracks); point_status: n_points int32 (only TRACK_OK points take part) or None
    (all points); point_xyz: n_points x 3 float64 or None (no distance gate), max_dist: the gate; bridge: rows without a point
    may carry a merge; obs_point: F * cap int32 as extend_tracks returns it, or None -- all cuda.  in_place: node_point and
    obs_point are updated where they are and returned.  With N = F * cap -> dict of device tensors: point_remap n_points int32
    (the surviving id of every point), point_state n_points uint8 (MERGE_NONE, MERGE_SURVIVOR, MERGE_ABSORBED, MERGE_CONFLICT,
    MERGE_FAR), point_select n_points uint8 (1 at the survivors), node_point N int32, obs_point N int32 or None, point_len
    n_points int32, totals 6 int32 (MERGED groups, ABSORBED points, CONFLICT groups, FAR groups, nodes whose point changed, points
    in CONFLICT or FAR groups); nothing is synchronised and nothing is read back: obs_cam / obs_xy of extend_tracks stay valid,
    and triangulate_tracks with point_select = point_select gives the survivors their coordinates from all of their
    observations."""
    import torch
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, pair_q, pair_t, idx1, node_point))
    F, cap, P = counts.numel(), int(cap), pair_q.shape[0]
    N, dev, n_points = F * cap, counts.device, int(n_points)
    assert pair_t.shape[0] == P and idx1.numel() == P * cap and node_point.numel() == N and n_points >= 0
    assert inlier is None or (inlier.is_cuda and inlier.dtype == torch.uint8 and inlier.is_contiguous() and inlier.numel() == P * cap)
    assert point_status is None or (point_status.is_cuda and point_status.dtype == torch.int32 and point_status.is_contiguous() and
                                    point_status.numel() == n_points)
    assert point_xyz is None or (point_xyz.is_cuda and point_xyz.dtype == torch.float64 and point_xyz.is_contiguous() and
                                 point_xyz.numel() == 3 * n_points)
    assert obs_point is None or (obs_point.is_cuda and obs_point.dtype == torch.int32 and obs_point.is_contiguous() and
                                 obs_point.numel() == N)
    out = {"point_remap": torch.empty(n_points, dtype=torch.int32, device=dev),
           "point_state": torch.empty(n_points, dtype=torch.uint8, device=dev),
           "point_select": torch.empty(n_points, dtype=torch.uint8, device=dev),
           "node_point": node_point if in_place else torch.empty(N, dtype=torch.int32, device=dev),
           "obs_point": None if obs_point is None else (obs_point if in_place else torch.empty(N, dtype=torch.int32, device=dev)),
           "point_len": torch.empty(n_points, dtype=torch.int32, device=dev),
           "totals": torch.empty(6, dtype=torch.int32, device=dev)}
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    q = lambda t: None if t is None else p(t)  # (NULL means "not given", also when the array holds nothing)
    ctx.check(hip.lib.gh_merge_points_dev(ctx.h, p(counts), F, cap, p(pair_q), p(pair_t), P, p(idx1), _p(inlier), p(node_point),
                                          n_points, q(point_status), q(point_xyz), C.c_double(float(max_dist)), 1 if bridge else 0,
                                          q(obs_point), *(q(out[k]) for k in out)))
    return out


def point_desc_default_params():
    """gh_point_desc_default_params -> hip.PointDescParams (scale_factor, n_levels, max_views)."""
    p = hip.PointDescParams()
    hip.lib.gh_point_desc_default_params(C.byref(p))
    return p


DESCRIBE_OUTPUTS = ("point_state", "point_desc", "point_obs", "point_views", "point_normal", "point_dist", "totals")


def describe_points(ctx: hip.Context, kps, desc, counts, cam_pose, obs_cam, obs_point, obs_node, n_points, point_xyz, obs_use=None,
                    point_status=None, point_select=None, params=None, out=None):
    """gh_describe_points_dev, the call after triangulate_tracks (and after extend_tracks / merge_points, for the points that
    changed): every map point gets the descriptor of the observation closest to its other observations, the mean direction it
    was seen from and the distance range its reference keypoint's octave predicts -- what a search by projection needs.
    kps: F x cap x 7 float32 view of the KeyPoint records, desc: F x cap x 32 uint8, counts: F int32, cam_pose: F x 7 float64
    T_wc; obs_cam / obs_point / obs_node: n_obs int32 as link_tracks / extend_tracks / merge_points leave them; n_points: the
    capacity of the point arrays; point_xyz: n_points x 3 float64; obs_use: n_obs uint8 (obs_good of triangulate_tracks) or
    None; point_status: n_points int32 (only TRACK_OK points are described) or None; point_select: n_points uint8 or None (all
    points) -- all cuda; params: hip.PointDescParams or None (the defaults); out: the dict an earlier call returned, to be
    refreshed where point_select says so (the other points keep what they hold), or None for zeroed arrays.  -> dict of device
    tensors: point_state n_points uint8 (PDESC_*), point_desc n_points x 32 uint8, point_obs n_points x 2 int32 (the chosen
    observation, the reference observation), point_views n_points int32, point_normal n_points x 3 and point_dist n_points x 2
    float64 (min, max), totals 4 int32 (OK, EMPTY, NOT_OK points, OK points with more than max_views observations); nothing is
    synchronised and nothing is read back."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    F, cap = kps.shape[0], kps.shape[1]
    N, dev, n_points = F * cap, kps.device, int(n_points)
    assert desc.is_cuda and desc.dtype == torch.uint8 and desc.is_contiguous() and desc.numel() == 32 * N
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (counts, obs_cam, obs_point, obs_node))
    n_obs = obs_cam.numel()
    assert counts.numel() == F and obs_point.numel() == n_obs and obs_node.numel() == n_obs and n_points >= 0
    assert cam_pose.is_cuda and cam_pose.dtype == torch.float64 and cam_pose.is_contiguous() and cam_pose.numel() == 7 * F
    assert point_xyz.is_cuda and point_xyz.dtype == torch.float64 and point_xyz.is_contiguous() and point_xyz.numel() == 3 * n_points
    assert obs_use is None or (obs_use.is_cuda and obs_use.dtype == torch.uint8 and obs_use.is_contiguous() and obs_use.numel() == n_obs)
    assert point_status is None or (point_status.is_cuda and point_status.dtype == torch.int32 and point_status.is_contiguous() and
                                    point_status.numel() == n_points)
    assert point_select is None or (point_select.is_cuda and point_select.dtype == torch.uint8 and point_select.is_contiguous() and
                                    point_select.numel() == n_points)
    shapes = {"point_state": ((n_points,), torch.uint8), "point_desc": ((n_points, 32), torch.uint8),
              "point_obs": ((n_points, 2), torch.int32), "point_views": ((n_points,), torch.int32),
              "point_normal": ((n_points, 3), torch.float64), "point_dist": ((n_points, 2), torch.float64),
              "totals": ((4,), torch.int32)}
    if out is None:
        out = {k: torch.zeros(shape, dtype=dtype, device=dev) for k, (shape, dtype) in shapes.items()}
    else:
        assert list(out) == list(DESCRIBE_OUTPUTS)
        assert all(out[k].is_cuda and out[k].dtype == dtype and out[k].is_contiguous() and tuple(out[k].shape) == shape
                   for k, (shape, dtype) in shapes.items())
    prm = params if params is not None else point_desc_default_params()
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    ctx.check(hip.lib.gh_describe_points_dev(ctx.h, p(kps), p(desc), p(counts), F, cap, p(cam_pose), p(obs_cam), p(obs_point),
                                             p(obs_node), _p(obs_use), n_obs, n_points, p(point_xyz), _p(point_status),
                                             _p(point_select), C.byref(prm), *(p(out[k]) for k in DESCRIBE_OUTPUTS)))
    return out


def search_default_params():
    """gh_search_default_params -> hip.SearchParams."""
    p = hip.SearchParams()
    hip.lib.gh_search_default_params(C.byref(p))
    return p


SEARCH_OUTPUTS = ("row_point", "row_inlier", "row_dist", "frame_totals", "totals")
SEARCH_VERDICTS = ("HELD", "BEHIND", "OUTSIDE", "RANGE", "ANGLE", "NO_CANDIDATE", "WEAK", "RATIO", "LOST", "WON")


def search_projection(ctx: hip.Context, kps, desc, counts, cam_pose, frame_search, n_points, point_xyz, summaries, intrinsics, size,
                      node_point=None, row_point=None, row_inlier=None, point_status=None, point_select=None, params=None,
                      in_place=False):
    """gh_search_projection_dev, the call between localize_pairs and extend_tracks: the map's points are projected into the
    frames marked in frame_search and matched against the keypoints that have no point yet, in a window around the projection.
    kps, desc, counts, cam_pose, n_points, point_xyz, point_status, point_select as describe_points takes them (cam_pose may be
    the poses of localize_pairs); frame_search: F uint8; summaries: the dict describe_points returned (point_views, point_desc,
    point_normal, point_dist are read); intrinsics: fx, fy, cx, cy; size: (width, height); node_point: F * cap int32 (the map) or
    None; row_point F * cap int32 and row_inlier F * cap uint8: the claims of localize_pairs, or both None -- all cuda; params:
    hip.SearchParams or None (the defaults); in_place: the claims are updated where they are.  -> dict of device tensors:
    row_point N int32 and row_inlier N uint8 (the claims with the search's winners added: what extend_tracks takes), row_dist N
    uint16 (the Hamming distance of a winner, 0xFFFF elsewhere), frame_totals F x 10 int32 (the pairs per verdict,
    SEARCH_VERDICTS), totals 12 int32 (the column sums, the searched frames, the searchable points); nothing is synchronised and
    nothing is read back."""
    import torch
    assert kps.is_cuda and kps.dtype == torch.float32 and kps.is_contiguous() and kps.dim() == 3 and kps.shape[2] == 7
    F, cap = kps.shape[0], kps.shape[1]
    N, dev, n_points = F * cap, kps.device, int(n_points)
    assert desc.is_cuda and desc.dtype == torch.uint8 and desc.is_contiguous() and desc.numel() == 32 * N
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == F
    assert cam_pose.is_cuda and cam_pose.dtype == torch.float64 and cam_pose.is_contiguous() and cam_pose.numel() == 7 * F
    assert frame_search.is_cuda and frame_search.dtype == torch.uint8 and frame_search.is_contiguous() and frame_search.numel() == F
    assert point_xyz.is_cuda and point_xyz.dtype == torch.float64 and point_xyz.is_contiguous() and point_xyz.numel() == 3 * n_points
    want = {"point_views": (torch.int32, n_points), "point_desc": (torch.uint8, 32 * n_points),
            "point_normal": (torch.float64, 3 * n_points), "point_dist": (torch.float64, 2 * n_points)}
    assert all(summaries[k].is_cuda and summaries[k].dtype == dt and summaries[k].is_contiguous() and summaries[k].numel() == n
               for k, (dt, n) in want.items())
    for t, dt, n in ((node_point, torch.int32, N), (row_point, torch.int32, N), (row_inlier, torch.uint8, N),
                     (point_status, torch.int32, n_points), (point_select, torch.uint8, n_points)):
        assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == n)
    assert (row_point is None) == (row_inlier is None) and not (in_place and row_point is None)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    out = {"row_point": row_point if in_place else torch.empty(N, dtype=torch.int32, device=dev),
           "row_inlier": row_inlier if in_place else torch.empty(N, dtype=torch.uint8, device=dev),
           "row_dist": torch.empty(N, dtype=torch.uint16, device=dev),
           "frame_totals": torch.empty((F, 10), dtype=torch.int32, device=dev),
           "totals": torch.empty(12, dtype=torch.int32, device=dev)}
    prm = params if params is not None else search_default_params()
    # (an empty tensor has no storage: its pointer is 0, and the entry wants its arrays even when they hold nothing)
    p = lambda t: C.c_void_p(t.data_ptr() or 256)
    q = lambda t: None if t is None else p(t)  # (NULL means "not given", also when the array holds nothing)
    ctx.check(hip.lib.gh_search_projection_dev(ctx.h, p(kps), p(desc), p(counts), F, cap, p(cam_pose), p(frame_search), q(node_point),
                                               q(row_point), q(row_inlier), n_points, p(point_xyz), q(point_status), q(point_select),
                                               *(p(summaries[k]) for k in want), C.c_double(fx), C.c_double(fy), C.c_double(cx),
                                               C.c_double(cy), int(size[0]), int(size[1]), C.byref(prm),
                                               *(p(out[k]) for k in SEARCH_OUTPUTS)))
    return out


def triangulate(ctx: hip.Context, ref2cur_pose, ref_dir, cur_dir):
    """Midpoint triangulation (GSLAM::Estimator::trianglate); ref2cur_pose: 7 doubles (one pose for all) or n x 7."""
    T = np.ascontiguousarray(ref2cur_pose, dtype=np.float64)
    d1 = np.ascontiguousarray(ref_dir, dtype=np.float64).reshape(-1, 3)
    d2 = np.ascontiguousarray(cur_dir, dtype=np.float64).reshape(-1, 3)
    n = d1.shape[0]
    out = np.zeros((n, 3))
    ok = np.zeros(max(n, 1), np.uint8)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.check(hip.lib.gh_triangulate(ctx.h, pv(T), 7 if T.ndim == 2 else 0, pv(d1), pv(d2), n, pv(out), pv(ok)))
    return out, ok[:n].astype(bool)
