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
from .devargs import alloc, defaults, dev, keypoints, pair_arrays, pinhole, ptr, ptr_array, ptr_opt, require

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


def batch_tile_rows(model):
    """gh_ransac_batch_tile_rows: correspondences the batched scoring kernel stages at a time (<= 0: unknown model)."""
    return int(hip.lib.gh_ransac_batch_tile_rows(int(model)))


def estimate_batch(ctx: hip.Context, model, src, dst, offsets, threshold, seed, thresholds=None, seeds=None):
    """gh_ransac_batch_dev.  src, dst: rows x dim float64 (cuda); offsets: nproblems + 1 int32 (cuda), problem p owns rows
    offsets[p] .. offsets[p + 1] - 1; thresholds (float64) / seeds (int64 holding the uint64 bits) per problem or None for
    the scalars.  -> (models nproblems x 12 float64, mask rows uint8, inliers nproblems int32), all on the device; nothing
    is synchronised.  Problem p equals estimate(ctx, model, src_p, dst_p, threshold_p, seed_p)."""
    dev("src", src, "float64")
    dev("dst", dst, "float64")
    dev("offsets", offsets, "int32")
    require(offsets.numel() >= 1, "offsets: empty, expected nproblems + 1 entries")
    n = offsets.numel() - 1
    dev("thresholds", thresholds, "float64", n, optional=True)
    dev("seeds", seeds, "int64", n, optional=True)
    out = alloc(src.device, {"models": ((n, 12), "float64"),
                             "mask": (src.shape[0], "uint8", True),  # (rows past offsets[n], if any, belong to nobody)
                             "inliers": (n, "int32")})
    ctx.check(hip.lib.gh_ransac_batch_dev(ctx.h, int(model), ptr(src), ptr(dst), ptr(offsets), n, C.c_double(threshold),
                                          ptr(thresholds), C.c_uint64(seed), ptr(seeds), *map(ptr, out.values())))
    return tuple(out.values())


def _pair_io(kps, counts, pair_q, pair_t, idx1, keep):
    """The inputs of the pair entries, checked, and the output tensors both have, in the order of the C arguments
    -> (P, cap, out)."""
    F, cap = keypoints(kps)
    P = pair_arrays(counts, F, cap, pair_q, pair_t, idx1, keep)
    out = alloc(kps.device, {"models": ((P, 12), "float64"), "inlier": ((P, cap), "uint8"),
                             "n_corr": (P, "int32"), "inliers": (P, "int32")})
    return P, cap, out


def estimate_pairs(ctx: hip.Context, model, kps, counts, pair_q, pair_t, idx1, keep, threshold, seed):
    """gh_ransac_pairs_dev, the call after BFMatcher.match_pairs / mask.  kps: F x cap x 7 float32 view of the KeyPoint
    records, counts: F int32, pair_q / pair_t: P int32, idx1: P x cap int32, keep: P x cap uint8 or None (all cuda).
    model: HOMOGRAPHY, AFFINE2D or FUNDAMENTAL.  -> (models P x 12, inlier P x cap uint8, n_corr P int32, inliers P int32)
    on the device; pair p equals estimate() on the rows correspondences_from_matches lists for it."""
    P, cap, out = _pair_io(kps, counts, pair_q, pair_t, idx1, keep)
    ctx.check(hip.lib.gh_ransac_pairs_dev(ctx.h, int(model), ptr(kps), ptr(counts), cap, ptr(pair_q), ptr(pair_t), P, ptr(idx1),
                                          ptr(keep), C.c_double(threshold), C.c_uint64(seed), *map(ptr, out.values())))
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
    return defaults(None, hip.TwoViewParams, hip.lib.gh_two_view_default_params)


def two_view_batch(ctx: hip.Context, E, src, dst, offsets, mask=None, params=None):
    """gh_two_view_batch_dev.  E: nproblems x e_stride float64 (cuda, e_stride >= 9: the models of estimate_batch go in as they
    are), src / dst: rows x 2 float64 normalised coordinates, offsets: nproblems + 1 int32, mask: rows uint8 or None (all rows
    take part).  -> (poses nproblems x 7 [qx qy qz qw tx ty tz] ref -> cur, points rows x 3 in the reference frame, good rows
    uint8, counts nproblems x 4 int32, n_used nproblems int32, status nproblems int32: TWO_VIEW_*), all on the device;
    nothing is synchronised."""
    dev("E", E, "float64")
    require(E.dim() == 2 and E.shape[1] >= 9, "E: shape %s, expected nproblems x e_stride with e_stride >= 9" % (tuple(E.shape),))
    dev("src", src, "float64")
    dev("dst", dst, "float64")
    n, rows = E.shape[0], src.shape[0]
    dev("offsets", offsets, "int32", n + 1)
    dev("mask", mask, "uint8", rows, optional=True)
    prm = defaults(params, hip.TwoViewParams, hip.lib.gh_two_view_default_params)
    out = alloc(src.device, {"poses": ((n, 7), "float64"),
                             "points": ((rows, 3), "float64", True),  # (rows past offsets[n], if any, belong to nobody)
                             "good": (rows, "uint8", True), "counts": ((n, 4), "int32"),
                             "n_used": (n, "int32"), "status": (n, "int32")})
    ctx.check(hip.lib.gh_two_view_batch_dev(ctx.h, ptr(E), int(E.shape[1]), ptr(src), ptr(dst), ptr(offsets), n, ptr(mask),
                                            C.byref(prm), *map(ptr, out.values())))
    return tuple(out.values())


def two_view_pairs(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, keep, intrinsics, threshold, seed, params=None):
    """gh_two_view_pairs_dev, the call after BFMatcher.match_pairs / mask for a calibrated camera.  kps .. keep as
    estimate_pairs takes them; intrinsics: (fx, fy, cx, cy); threshold: of the essential fit, in normalised units.
    -> dict of device tensors: models P x 12, inlier P x cap uint8, n_corr P, inliers P, poses P x 7, points P x cap x 3,
    good P x cap uint8, votes P x 4 (the four candidate counts), status P.  Pair p equals estimate_batch(ESSENTIAL) and
    two_view_batch on the normalised rows correspondences_from_matches lists for it, scattered back to query rows."""
    P, cap, out = _pair_io(kps, counts, pair_q, pair_t, idx1, keep)
    prm = defaults(params, hip.TwoViewParams, hip.lib.gh_two_view_default_params)
    out.update(alloc(kps.device, {"poses": ((P, 7), "float64"), "points": ((P, cap, 3), "float64"),
                                  "good": ((P, cap), "uint8"), "votes": ((P, 4), "int32"), "status": (P, "int32")}))
    ctx.check(hip.lib.gh_two_view_pairs_dev(ctx.h, ptr(kps), ptr(counts), cap, ptr(pair_q), ptr(pair_t), P, ptr(idx1), ptr(keep),
                                            *pinhole(intrinsics), C.c_double(threshold), C.c_uint64(seed), C.byref(prm),
                                            *map(ptr, out.values())))
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


def _pnp_outputs(n, want_information, chain):
    """The outputs of a PnP batch of n problems, without the row bytes (chain: with the fit's outputs in front and a summary per
    round), in the order of the C arguments."""
    size = C.sizeof(hip.PnpBatchSummary)
    spec = {"models": ((n, 12), "float64"), "ransac_inliers": (n, "int32")} if chain else {}
    spec.update({"poses": ((n, 7), "float64"), "info": ((n, 36), "float64") if want_information else None,
                 "summaries": ((n, 2, size) if chain else (n, size), "uint8")})
    return spec


def _pnp_io(xyz, xy, offsets, want_information, chain=False):
    """The inputs both PnP batch entries share, checked, and their output tensors in the order of the C arguments (chain: with
    the fit's outputs in front and a summary per round) -> (nproblems, rows, out)."""
    rows = dev("xyz", xyz, "float64").shape[0]
    require(xyz.numel() == 3 * rows, "xyz: shape %s, expected rows x 3" % (tuple(xyz.shape),))
    dev("xy", xy, "float64", 2 * rows)
    dev("offsets", offsets, "int32")
    require(offsets.numel() >= 1, "offsets: empty, expected nproblems + 1 entries")
    n = offsets.numel() - 1
    spec = _pnp_outputs(n, want_information, chain)
    spec.update({"inlier": (rows, "uint8", True),  # (rows no range owns belong to nobody)
                 "n_inliers": (n, "int32")})
    return n, rows, alloc(xyz.device, spec)


def pnp_refine_batch(ctx: hip.Context, xyz, xy, offsets, start, mask=None, dof=63, options=None, min_rows=0,
                     inlier_threshold=-1.0, want_information=False):
    """gh_pnp_refine_batch_dev.  xyz: rows x 3, xy: rows x 2 float64 (cuda); offsets: nproblems + 1 int32; start: nproblems x 7
    (T_wc poses) or nproblems x 12 (models of estimate_batch(PNP)) float64; mask: rows uint8 or None (all rows take part);
    options: hip.BaOptions or None for the defaults.  -> dict of device tensors: poses nproblems x 7, info nproblems x 36 or
    None, summaries nproblems x 32 uint8 (view the host copy as SUMMARY_DTYPE), inlier rows uint8, n_inliers nproblems int32;
    nothing is synchronised.  A problem that is optimised equals ba.pnp on its participating rows, bit for bit."""
    n, rows, out = _pnp_io(xyz, xy, offsets, want_information)
    dev("start", start, "float64")
    require(start.dim() == 2 and start.shape[0] == n and start.shape[1] in (7, 12),
            "start: shape %s, expected %d x 7 or %d x 12" % (tuple(start.shape), n, n))
    dev("mask", mask, "uint8", rows, optional=True)
    opt = defaults(options, hip.BaOptions, hip.lib.gh_ba_default_options)
    ctx.check(hip.lib.gh_pnp_refine_batch_dev(ctx.h, ptr(xyz), ptr(xy), ptr(offsets), n, rows, ptr(mask), ptr(start),
                                              int(start.shape[1]), int(dof), C.byref(opt), int(min_rows),
                                              C.c_double(inlier_threshold), *map(ptr, out.values())))
    return out


def pnp_batch(ctx: hip.Context, xyz, xy, offsets, ransac_threshold, seed, inlier_threshold, dof=63, options=None, min_rows=0,
              want_information=False):
    """gh_pnp_batch_dev, the call after a 3D-2D gather: estimate_batch(PNP), pnp_refine_batch on its inliers from its models,
    pnp_refine_batch again on the rows within inlier_threshold from the first round's poses.  -> dict of device tensors:
    models nproblems x 12, ransac_inliers nproblems, poses nproblems x 7, info nproblems x 36 or None, summaries
    nproblems x 2 x 32 uint8 (round 1, round 2), inlier rows uint8, n_inliers nproblems; nothing is synchronised."""
    n, rows, out = _pnp_io(xyz, xy, offsets, want_information, chain=True)
    opt = defaults(options, hip.BaOptions, hip.lib.gh_ba_default_options)
    ctx.check(hip.lib.gh_pnp_batch_dev(ctx.h, ptr(xyz), ptr(xy), ptr(offsets), n, rows, C.c_double(ransac_threshold),
                                       C.c_uint64(seed), int(dof), C.byref(opt), int(min_rows), C.c_double(inlier_threshold),
                                       *map(ptr, out.values())))
    return out


def track_default_params():
    """gh_track_default_params -> hip.TrackParams (min_parallax_cos, max_reproj, min_views, max_drops)."""
    return defaults(None, hip.TrackParams, hip.lib.gh_track_default_params)


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
    n_cams = dev("cam_pose", cam_pose, "float64", multiple_of=7).numel() // 7
    n_obs, n_points = dev("obs_cam", obs_cam, "int32").numel(), int(n_points)
    require(n_points >= 0, "n_points: %d" % n_points)
    dev("obs_point", obs_point, "int32", n_obs)
    dev("obs_xy", obs_xy, "float64", 2 * n_obs)
    dev("obs_use", obs_use, "uint8", n_obs, optional=True)
    dev("point_select", point_select, "uint8", n_points, optional=True)
    dev("point_xyz", point_xyz, "float64", 3 * n_points, optional=True)
    prm = defaults(params, hip.TrackParams, hip.lib.gh_track_default_params)
    out = alloc(cam_pose.device, {"point_xyz": ((n_points, 3), "float64", True) if point_xyz is None else point_xyz,
                                  "status": (n_points, "int32"), "n_good": (n_points, "int32"),
                                  "obs_good": (n_obs, "uint8")})
    ctx.check(hip.lib.gh_triangulate_tracks_dev(ctx.h, ptr_array(cam_pose), n_cams, ptr_array(obs_cam), ptr_array(obs_point),
                                                ptr_array(obs_xy), n_obs, n_points, ptr(obs_use), ptr(point_select), C.byref(prm),
                                                *map(ptr_array, out.values())))
    return out


def _pair_args(counts, F, cap, pair_q, pair_t, P, idx1, mask):
    """The C arguments counts .. keep / inlier of the map entries: the arrays are wanted even when they hold nothing, the mask
    is NULL when it is not given."""
    return ptr_array(counts), F, cap, ptr_array(pair_q), ptr_array(pair_t), P, ptr_array(idx1), ptr(mask)


def _obs_outputs(N):
    """The node labels and the observation list that link_tracks and extend_tracks write, in the order of the C arguments."""
    return {"node_point": (N, "int32"), "obs_cam": (N, "int32"), "obs_point": (N, "int32"),
            "obs_xy": ((N, 2), "float64"), "obs_node": (N, "int32")}


def link_tracks(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, inlier, intrinsics, min_views=2):
    """gh_link_tracks_dev, the call between the pair entries and triangulate_tracks.  kps: F x cap x 7 float32 view of the
    KeyPoint records, counts: F int32, pair_q / pair_t: P int32, idx1: P x cap int32, inlier: P x cap uint8 or None (all rows):
    keep of BFMatcher.mask, inlier of estimate_pairs, inlier / good of two_view_pairs (all cuda); intrinsics: (fx, fy, cx, cy).
    With N = F * cap -> dict of device tensors: node_point N int32 (a point id, LINK_SHORT, LINK_CONFLICT or LINK_NO_ROW),
    obs_cam / obs_point / obs_node N int32 and obs_xy N x 2 float64 (padded past n_obs with -1 and zeros), point_len N // 2
    int32, totals 4 int32 (n_obs, n_points, CONFLICT components, SHORT components of two nodes or more); nothing is
    synchronised and nothing is read back: obs_cam, obs_point, obs_xy go to triangulate_tracks as they are, with
    n_points = N // 2."""
    F, cap = keypoints(kps)
    P = pair_arrays(counts, F, cap, pair_q, pair_t, idx1, inlier, "inlier")
    N = F * cap
    out = alloc(kps.device, {**_obs_outputs(N), "point_len": (N // 2, "int32"), "totals": (4, "int32")})
    ctx.check(hip.lib.gh_link_tracks_dev(ctx.h, ptr_array(kps), *_pair_args(counts, F, cap, pair_q, pair_t, P, idx1, inlier),
                                         *pinhole(intrinsics), int(min_views), *map(ptr_array, out.values())))
    return out


def _gather_io(kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status):
    """The inputs of the two map entries, checked, and the gather's output tensors in the order of the C arguments
    -> (F, cap, P, n_points, out)."""
    F, cap = keypoints(kps)
    P = pair_arrays(counts, F, cap, pair_q, pair_t, idx1, keep)
    N = F * cap
    dev("node_point", node_point, "int32", N)
    n_points = dev("point_xyz", point_xyz, "float64", multiple_of=3).numel() // 3
    dev("point_status", point_status, "int32", n_points, optional=True)
    out = alloc(kps.device, {"row_point": (N, "int32"), "offsets": (F + 1, "int32"), "xyz": ((N, 3), "float64"),
                             "xy": ((N, 2), "float64"), "corr_node": (N, "int32"), "totals": (4, "int32")})
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
    ctx.check(hip.lib.gh_pnp_gather_pairs_dev(ctx.h, ptr_array(kps), *_pair_args(counts, F, cap, pair_q, pair_t, P, idx1, keep),
                                              ptr_array(node_point), n_points, ptr_array(point_xyz), ptr(point_status),
                                              *pinhole(intrinsics), *map(ptr_array, out.values())))
    return out


def localize_pairs(ctx: hip.Context, kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status, intrinsics,
                   ransac_threshold, seed, inlier_threshold, dof=63, options=None, min_rows=0, want_information=False):
    """gh_localize_pairs_dev: every frame registered against the map in one call -- gather_map_matches, pnp_batch on its arrays
    (one problem per frame), and the inlier bytes of the last round scattered back to keypoint rows.  Inputs as
    gather_map_matches and pnp_batch take them.  -> dict of device tensors: the gather's (row_point, offsets, xyz, xy, corr_node,
    totals), then models F x 12, ransac_inliers F, poses F x 7, info F x 36 or None, summaries F x 2 x 32 uint8 (view the host
    copy as SUMMARY_DTYPE), row_inlier F * cap uint8 (1 where the row's correspondence is an inlier of the last round); nothing
    is synchronised.  row_point and row_inlier are what extends the tracks with the new observations."""
    F, cap, P, n_points, out = _gather_io(kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status)
    out.update(alloc(kps.device, {**_pnp_outputs(F, want_information, chain=True), "row_inlier": (F * cap, "uint8")}))
    opt = defaults(options, hip.BaOptions, hip.lib.gh_ba_default_options)
    # (ptr_opt on the outputs: info is None when it was not asked for)
    ctx.check(hip.lib.gh_localize_pairs_dev(ctx.h, ptr_array(kps), *_pair_args(counts, F, cap, pair_q, pair_t, P, idx1, keep),
                                            ptr_array(node_point), n_points, ptr_array(point_xyz), ptr(point_status),
                                            *pinhole(intrinsics), C.c_double(ransac_threshold), C.c_uint64(seed), int(dof),
                                            C.byref(opt), int(min_rows), C.c_double(inlier_threshold),
                                            *map(ptr_opt, out.values())))
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
    F, cap = keypoints(kps)
    P = pair_arrays(counts, F, cap, pair_q, pair_t, idx1, inlier, "inlier")
    N, n_points = F * cap, int(n_points)
    require(n_points >= 0, "n_points: %d" % n_points)
    dev("node_point", node_point, "int32", N, optional=True)
    require((row_point is None) == (row_inlier is None), "row_point and row_inlier: both or neither")
    dev("row_point", row_point, "int32", N, optional=True)
    dev("row_inlier", row_inlier, "uint8", N, optional=True)
    PC = n_points + N // 2
    out = alloc(kps.device, {**_obs_outputs(N), "point_len": (PC, "int32"), "point_new": (PC, "uint8"),
                             "point_grew": (PC, "uint8"), "totals": (6, "int32")})
    # (ptr_opt: NULL means "not given" for these three, also when N == 0)
    ctx.check(hip.lib.gh_extend_tracks_dev(ctx.h, ptr_array(kps), *_pair_args(counts, F, cap, pair_q, pair_t, P, idx1, inlier),
                                           ptr_opt(node_point), n_points, ptr_opt(row_point), ptr_opt(row_inlier),
                                           *pinhole(intrinsics), int(min_views), *map(ptr_array, out.values())))
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
    F, cap = dev("counts", counts, "int32").numel(), int(cap)
    P = pair_arrays(counts, F, cap, pair_q, pair_t, idx1, inlier, "inlier")
    N, n_points = F * cap, int(n_points)
    require(n_points >= 0, "n_points: %d" % n_points)
    dev("node_point", node_point, "int32", N)
    dev("point_status", point_status, "int32", n_points, optional=True)
    dev("point_xyz", point_xyz, "float64", 3 * n_points, optional=True)
    dev("obs_point", obs_point, "int32", N, optional=True)
    out = alloc(counts.device, {"point_remap": (n_points, "int32"), "point_state": (n_points, "uint8"),
                                "point_select": (n_points, "uint8"),
                                "node_point": node_point if in_place else (N, "int32"),
                                "obs_point": obs_point if in_place or obs_point is None else (N, "int32"),
                                "point_len": (n_points, "int32"), "totals": (6, "int32")})
    # (ptr_opt: NULL means "not given", also when the array holds nothing; obs_point of the outputs is None with its input)
    ctx.check(hip.lib.gh_merge_points_dev(ctx.h, *_pair_args(counts, F, cap, pair_q, pair_t, P, idx1, inlier),
                                          ptr_array(node_point), n_points, ptr_opt(point_status), ptr_opt(point_xyz),
                                          C.c_double(float(max_dist)), 1 if bridge else 0, ptr_opt(obs_point),
                                          *map(ptr_opt, out.values())))
    return out


def point_desc_default_params():
    """gh_point_desc_default_params -> hip.PointDescParams (scale_factor, n_levels, max_views)."""
    return defaults(None, hip.PointDescParams, hip.lib.gh_point_desc_default_params)


DESCRIBE_OUTPUTS = ("point_state", "point_desc", "point_obs", "point_views", "point_normal", "point_dist", "totals")


def _frame_io(kps, desc, counts, cam_pose, n_points, point_xyz, point_status, point_select):
    """The frame and point arrays describe_points and search_projection share, checked -> (F, cap, n_points)."""
    F, cap = keypoints(kps)
    n_points = int(n_points)
    require(n_points >= 0, "n_points: %d" % n_points)
    dev("desc", desc, "uint8", 32 * F * cap)
    dev("counts", counts, "int32", F)
    dev("cam_pose", cam_pose, "float64", 7 * F)
    dev("point_xyz", point_xyz, "float64", 3 * n_points)
    dev("point_status", point_status, "int32", n_points, optional=True)
    dev("point_select", point_select, "uint8", n_points, optional=True)
    return F, cap, n_points


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
    F, cap, n_points = _frame_io(kps, desc, counts, cam_pose, n_points, point_xyz, point_status, point_select)
    n_obs = dev("obs_cam", obs_cam, "int32").numel()
    dev("obs_point", obs_point, "int32", n_obs)
    dev("obs_node", obs_node, "int32", n_obs)
    dev("obs_use", obs_use, "uint8", n_obs, optional=True)
    spec = dict(zip(DESCRIBE_OUTPUTS, (((n_points,), "uint8", True), ((n_points, 32), "uint8", True),
                                       ((n_points, 2), "int32", True), ((n_points,), "int32", True),
                                       ((n_points, 3), "float64", True), ((n_points, 2), "float64", True),
                                       ((4,), "int32", True))))
    if out is None:
        out = alloc(kps.device, spec)
    else:
        require(list(out) == list(DESCRIBE_OUTPUTS), "out: keys %s, expected %s" % (list(out), list(DESCRIBE_OUTPUTS)))
        for k, (shape, dtype, _) in spec.items():
            have = tuple(dev("out[%r]" % k, out[k], dtype).shape)
            require(have == shape, "out[%r]: shape %s, expected %s" % (k, have, shape))
    prm = defaults(params, hip.PointDescParams, hip.lib.gh_point_desc_default_params)
    ctx.check(hip.lib.gh_describe_points_dev(ctx.h, ptr_array(kps), ptr_array(desc), ptr_array(counts), F, cap, ptr_array(cam_pose),
                                             ptr_array(obs_cam), ptr_array(obs_point), ptr_array(obs_node), ptr(obs_use), n_obs,
                                             n_points, ptr_array(point_xyz), ptr(point_status), ptr(point_select), C.byref(prm),
                                             *map(ptr_array, out.values())))
    return out


def search_default_params():
    """gh_search_default_params -> hip.SearchParams."""
    return defaults(None, hip.SearchParams, hip.lib.gh_search_default_params)


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
    F, cap, n_points = _frame_io(kps, desc, counts, cam_pose, n_points, point_xyz, point_status, point_select)
    N = F * cap
    dev("frame_search", frame_search, "uint8", F)
    want = {"point_views": ("int32", n_points), "point_desc": ("uint8", 32 * n_points),
            "point_normal": ("float64", 3 * n_points), "point_dist": ("float64", 2 * n_points)}
    for k, (dtype, n) in want.items():
        dev("summaries[%r]" % k, summaries[k], dtype, n)
    dev("node_point", node_point, "int32", N, optional=True)
    dev("row_point", row_point, "int32", N, optional=True)
    dev("row_inlier", row_inlier, "uint8", N, optional=True)
    require((row_point is None) == (row_inlier is None), "row_point and row_inlier: both or neither")
    require(not (in_place and row_point is None), "in_place: there are no claims to update")
    out = alloc(kps.device, dict(zip(SEARCH_OUTPUTS, (row_point if in_place else (N, "int32"),
                                                      row_inlier if in_place else (N, "uint8"), (N, "uint16"),
                                                      ((F, 10), "int32"), (12, "int32")))))
    prm = defaults(params, hip.SearchParams, hip.lib.gh_search_default_params)
    # (ptr_opt: NULL means "not given", also when the array holds nothing)
    ctx.check(hip.lib.gh_search_projection_dev(ctx.h, ptr_array(kps), ptr_array(desc), ptr_array(counts), F, cap, ptr_array(cam_pose),
                                               ptr_array(frame_search), ptr_opt(node_point), ptr_opt(row_point), ptr_opt(row_inlier),
                                               n_points, ptr_array(point_xyz), ptr_opt(point_status), ptr_opt(point_select),
                                               *(ptr_array(summaries[k]) for k in want), *pinhole(intrinsics), int(size[0]),
                                               int(size[1]), C.byref(prm), *map(ptr_array, out.values())))
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
