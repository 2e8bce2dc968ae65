"""The contract of gh_extend_tracks_dev (include/gslam_hip.h) in plain Python: dicts, sets and lists, a textbook union-find,
Python floats for the normalisation (numpy.float32 -> float is the exact widening float -> double).  No numpy vector operation
that could hide an ordering.  Every output comes back at its full capacity, as the device writes it.  The edge rule is the one
of gh_link_tracks_dev and is taken from its restatement (track_link_restate.edges)."""
import track_link_restate as lr

SHORT, CONFLICT, NO_ROW, REJECTED = -1, -2, -3, -4  # GH_LINK_*, GH_EXT_REJECTED
MAPPED, CLAIMANT, FREE = "mapped", "claimant", "free"


def _clamp(c, cap):
    return 0 if c < 0 else (cap if c > cap else c)


def states(counts, n_frames, cap, node_point_in, n_points, row_point, row_inlier):
    """{existing node: (state, point or None)} in the order of checking of the contract."""
    out = {}
    for f in range(n_frames):
        for i in range(_clamp(int(counts[f]), cap)):
            n = f * cap + i
            if node_point_in is not None and 0 <= int(node_point_in[n]) < n_points:
                out[n] = (MAPPED, int(node_point_in[n]))
            elif row_point is not None and row_inlier is not None and int(row_inlier[n]) != 0 and 0 <= int(row_point[n]) < n_points:
                out[n] = (CLAIMANT, int(row_point[n]))
            else:
                out[n] = (FREE, None)
    return out


def verdicts(state, cap):
    """-> (adopted {node: point}, rejected set): a claimant is rejected when its frame holds a MAPPED node of its point or
    another claimant of it."""
    holders = {}  # (frame, point) -> [number of MAPPED nodes, number of claimants]
    for n, (s, c) in state.items():
        if s != FREE:
            holders.setdefault((n // cap, c), [0, 0])[0 if s == MAPPED else 1] += 1
    adopted, rejected = {}, set()
    for n, (s, c) in state.items():
        if s == CLAIMANT:
            mapped, claimants = holders[(n // cap, c)]
            if mapped > 0 or claimants > 1:
                rejected.add(n)
            else:
                adopted[n] = c
    return adopted, rejected


def free_components(state, edge_list):
    """{label: [nodes, ascending]} of the graph on the FREE nodes; only an edge with both ends FREE counts."""
    parent = {n: n for n, (s, _) in state.items() if s == FREE}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in edge_list:
        if a in parent and b in parent:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for n in sorted(parent):
        comps.setdefault(find(n), []).append(n)
    for label, nodes in comps.items():
        assert label == min(nodes) == nodes[0]
    return comps


def extend(kps_xy, counts, n_frames, cap, pair_q, pair_t, idx1, inlier, node_point_in, n_points, row_point, row_inlier, intrinsics,
           min_views):
    """kps_xy: n_frames x cap x 2 numpy float32; idx1 / inlier flat (inlier may be None); node_point_in, row_point, row_inlier:
    lists of N or None.  -> dict of lists: node_point, obs_cam, obs_point, obs_node (N each), obs_xy (N pairs), point_len,
    point_new, point_grew (PC each), totals (6); and for the tests `state`, `adopted`, `rejected`, `components`."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    N = n_frames * cap
    PC = n_points + N // 2
    state = states(counts, n_frames, cap, node_point_in, n_points, row_point, row_inlier)
    adopted, rejected = verdicts(state, cap)
    comps = free_components(state, lr.edges(counts, n_frames, cap, pair_q, pair_t, idx1, inlier))
    node_point = [NO_ROW] * N
    for n, (s, c) in state.items():
        if s == MAPPED:
            node_point[n] = c
        elif s == CLAIMANT:
            node_point[n] = REJECTED if n in rejected else c
    point_len, point_new, point_grew = [0] * PC, [0] * PC, [0] * PC
    n_total, n_conflict, n_short = n_points, 0, 0
    for label in sorted(comps):
        nodes = comps[label]
        cls = lr.classify(nodes, cap, min_views)
        if cls == lr.CONFLICT:
            n_conflict += 1
            cls = CONFLICT
        elif cls == lr.SHORT:
            n_short += 1 if len(nodes) >= 2 else 0
            cls = SHORT
        else:
            cls = n_total
            point_new[n_total] = 1
            n_total += 1
        for n in nodes:
            node_point[n] = cls
    for c in adopted.values():
        point_grew[c] = 1
    obs_cam, obs_point, obs_node, obs_xy = [-1] * N, [-1] * N, [-1] * N, [(0.0, 0.0)] * N
    k = 0
    for n in range(N):
        if node_point[n] >= 0:
            f, i = n // cap, n % cap
            x, y = float(kps_xy[f][i][0]), float(kps_xy[f][i][1])
            obs_cam[k], obs_point[k], obs_node[k] = f, node_point[n], n
            obs_xy[k] = ((x - cx) / fx, (y - cy) / fy)
            point_len[node_point[n]] += 1
            k += 1
    return dict(node_point=node_point, obs_cam=obs_cam, obs_point=obs_point, obs_xy=obs_xy, obs_node=obs_node, point_len=point_len,
                point_new=point_new, point_grew=point_grew, totals=[k, n_total, len(adopted), len(rejected), n_conflict, n_short],
                state=state, adopted=adopted, rejected=rejected, components=comps)
