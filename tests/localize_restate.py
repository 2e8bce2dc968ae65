"""The contract of gh_pnp_gather_pairs_dev (include/gslam_hip.h) in plain Python: dicts, sets and lists, Python floats for the
normalisation (numpy.float32 -> float is the exact widening float -> double).  No numpy vector operation that could hide an
ordering.  Every output comes back at its full capacity, as the device writes it.  scatter() is the last step of
gh_localize_pairs_dev."""

NO_POINT, AMBIGUOUS, NO_ROW, SHARED = -1, -2, -3, -4  # GH_LOC_*
TRACK_OK = 0                                          # GH_TRACK_OK


def _clamp(c, cap):
    return 0 if c < 0 else (cap if c > cap else c)


def candidates(counts, n_frames, cap, pair_q, pair_t, idx1, keep, node_point, n_points, point_status):
    """{node: set of candidate point ids} over all pairs.  idx1 / keep: flat, npairs * cap; keep / point_status may be None."""
    out = {}
    for p in range(len(pair_q)):
        fq, ft = int(pair_q[p]), int(pair_t[p])
        if not (0 <= fq < n_frames and 0 <= ft < n_frames) or fq == ft:
            continue
        for i in range(_clamp(int(counts[fq]), cap)):
            if keep is not None and int(keep[p * cap + i]) == 0:
                continue
            j = int(idx1[p * cap + i])
            if not 0 <= j < _clamp(int(counts[ft]), cap):
                continue
            c = int(node_point[ft * cap + j])
            if not 0 <= c < n_points:
                continue
            if point_status is not None and int(point_status[c]) != TRACK_OK:
                continue
            out.setdefault(fq * cap + i, set()).add(c)
    return out


def gather(kps_xy, counts, n_frames, cap, pair_q, pair_t, idx1, keep, node_point, point_xyz, point_status, intrinsics):
    """kps_xy: n_frames x cap x 2 numpy float32 (x, y of every record); point_xyz: list of n_points triples.  -> dict of lists:
    row_point, corr_node (N each), offsets (n_frames + 1), xyz (N triples), xy (N pairs), totals (4)."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    N, n_points = n_frames * cap, len(point_xyz)
    cand = candidates(counts, n_frames, cap, pair_q, pair_t, idx1, keep, node_point, n_points, point_status)
    row_point = [NO_ROW] * N
    claims = {}  # (frame, point) -> the nodes of the frame that claim the point
    for f in range(n_frames):
        for i in range(_clamp(int(counts[f]), cap)):
            n = f * cap + i
            S = cand.get(n, set())
            if not S:
                row_point[n] = NO_POINT
            elif min(S) != max(S):
                row_point[n] = AMBIGUOUS
            else:
                row_point[n] = min(S)
                claims.setdefault((f, min(S)), []).append(n)
    for nodes in claims.values():
        if len(nodes) >= 2:
            for n in nodes:
                row_point[n] = SHARED
    xyz, xy, corr_node = [(0.0, 0.0, 0.0)] * N, [(0.0, 0.0)] * N, [-1] * N
    offsets = [0] * (n_frames + 1)
    k = 0
    for f in range(n_frames):
        offsets[f] = k
        for i in range(cap):
            n = f * cap + i
            if row_point[n] >= 0:
                x, y = float(kps_xy[f][i][0]), float(kps_xy[f][i][1])
                xyz[k] = tuple(float(v) for v in point_xyz[row_point[n]])
                xy[k] = ((x - cx) / fx, (y - cy) / fy)
                corr_node[k] = n
                k += 1
    offsets[n_frames] = k
    totals = [k, row_point.count(AMBIGUOUS), row_point.count(SHARED), sum(offsets[f + 1] > offsets[f] for f in range(n_frames))]
    return dict(row_point=row_point, offsets=offsets, xyz=xyz, xy=xy, corr_node=corr_node, totals=totals)


def scatter(corr_node, n_corr, inlier, N):
    """row_inlier of gh_localize_pairs_dev: 1 exactly at the nodes whose correspondence is an inlier, 0 everywhere else."""
    row_inlier = [0] * N
    for k in range(n_corr):
        if int(inlier[k]):
            row_inlier[int(corr_node[k])] = 1
    return row_inlier
