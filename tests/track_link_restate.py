"""The contract of gh_link_tracks_dev (include/gslam_hip.h) in plain Python: dicts and lists, a textbook union-find, Python
floats for the normalisation (numpy.float32 -> float is the exact widening float -> double).  No numpy vector operation that
could hide an ordering.  Every output comes back at its full capacity, as the device writes it."""

SHORT, CONFLICT, NO_ROW = -1, -2, -3  # GH_LINK_*


def _clamp(c, cap):
    return 0 if c < 0 else (cap if c > cap else c)


def edges(counts, n_frames, cap, pair_q, pair_t, idx1, inlier):
    """The edge list (node, node) of the contract, in pair order then row order.  idx1 / inlier: flat, npairs * cap."""
    out = []
    for p in range(len(pair_q)):
        fq, ft = int(pair_q[p]), int(pair_t[p])
        if not (0 <= fq < n_frames and 0 <= ft < n_frames) or fq == ft:
            continue
        for i in range(_clamp(int(counts[fq]), cap)):
            if inlier is not None and int(inlier[p * cap + i]) == 0:
                continue
            j = int(idx1[p * cap + i])
            if 0 <= j < _clamp(int(counts[ft]), cap):
                out.append((fq * cap + i, ft * cap + j))
    return out


def components(counts, n_frames, cap, edge_list):
    """{label: [nodes, ascending]} over the existing nodes; the label is the smallest node of the component."""
    parent = {}
    for f in range(n_frames):
        for i in range(_clamp(int(counts[f]), cap)):
            parent[f * cap + i] = f * cap + i

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in edge_list:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for n in sorted(parent):
        comps.setdefault(find(n), []).append(n)
    for label, nodes in comps.items():
        assert label == min(nodes) == nodes[0]
    return comps


def classify(nodes, cap, min_views):
    frames = [n // cap for n in nodes]
    if len(set(frames)) != len(frames):
        return CONFLICT
    return SHORT if len(nodes) < min_views else 0


def link(kps_xy, counts, n_frames, cap, pair_q, pair_t, idx1, inlier, intrinsics, min_views):
    """kps_xy: n_frames x cap x 2 numpy float32 (x, y of every record); idx1 / inlier flat.  -> dict of lists: node_point,
    obs_cam, obs_point, obs_node (N each), obs_xy (N pairs), point_len (N // 2), totals (4), and `components` for the tests."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    N = n_frames * cap
    comps = components(counts, n_frames, cap, edges(counts, n_frames, cap, pair_q, pair_t, idx1, inlier))
    node_point = [NO_ROW] * N
    point_len = [0] * (N // 2)
    n_points = n_conflict = n_short = 0
    for label in sorted(comps):
        nodes = comps[label]
        cls = classify(nodes, cap, min_views)
        if cls == CONFLICT:
            n_conflict += 1
        elif cls == SHORT:
            n_short += 1 if len(nodes) >= 2 else 0
        else:
            cls = n_points
            point_len[n_points] = len(nodes)
            n_points += 1
        for n in nodes:
            node_point[n] = cls
    obs_cam, obs_point, obs_node, obs_xy = [-1] * N, [-1] * N, [-1] * N, [(0.0, 0.0)] * N
    k = 0
    for n in range(N):
        if node_point[n] >= 0:
            f, i = n // cap, n % cap
            x, y = float(kps_xy[f][i][0]), float(kps_xy[f][i][1])
            obs_cam[k], obs_point[k], obs_node[k] = f, node_point[n], n
            obs_xy[k] = ((x - cx) / fx, (y - cy) / fy)
            k += 1
    return dict(node_point=node_point, obs_cam=obs_cam, obs_point=obs_point, obs_xy=obs_xy, obs_node=obs_node, point_len=point_len,
                totals=[k, n_points, n_conflict, n_short], components=comps)
