"""The contract of gh_merge_points_dev (include/gslam_hip.h) in plain Python: dicts, sets and lists, a textbook union-find over
the keys ("p", point id) and ("n", node), Python floats for the gate, written (dx*dx + dy*dy) + dz*dz (every Python operation is
one IEEE double operation, rounded once).  No numpy vector operation that could hide an ordering.  Every output comes back at
its full capacity, as the device writes it.  The edge rule is the one of gh_link_tracks_dev and is taken from its restatement
(track_link_restate.edges)."""
import track_link_restate as lr

NONE, SURVIVOR, ABSORBED, CONFLICT, FAR = 0, 1, 2, 3, 4  # GH_MERGE_*
TRACK_OK = 0  # GH_TRACK_OK
HOLDER, BRIDGE, OUT = "holder", "bridge", "out"


def _clamp(c, cap):
    return 0 if c < 0 else (cap if c > cap else c)


def existing(counts, n_frames, cap):
    return [f * cap + i for f in range(n_frames) for i in range(_clamp(int(counts[f]), cap))]


def usable(p, point_status):
    return point_status is None or int(point_status[p]) == TRACK_OK


def classes(counts, n_frames, cap, node_point_in, n_points, point_status, bridge):
    """{existing node: (class, point or None)}."""
    out = {}
    for n in existing(counts, n_frames, cap):
        v = int(node_point_in[n])
        if 0 <= v < n_points:
            out[n] = (HOLDER, v) if usable(v, point_status) else (OUT, None)
        else:
            out[n] = (BRIDGE, None) if bridge else (OUT, None)
    return out


def d2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (dx * dx + dy * dy) + dz * dz


def groups_of(cls, n_points, point_status, edge_list):
    """{label: [points, ascending]} of the components with at least two points."""
    parent = {("p", p): ("p", p) for p in range(n_points) if usable(p, point_status)}
    parent.update({("n", n): ("n", n) for n, (c, _) in cls.items() if c == BRIDGE})

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def element(n):
        c, p = cls.get(n, (OUT, None))
        return ("p", p) if c == HOLDER else ("n", n) if c == BRIDGE else None

    for u, v in edge_list:
        a, b = element(u), element(v)
        if a is None or b is None or a == b:
            continue
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    comps = {}
    for key in parent:
        if key[0] == "p":
            comps.setdefault(find(key), []).append(key[1])
    return {min(pts): sorted(pts) for pts in comps.values() if len(pts) >= 2}


def merge(counts, n_frames, cap, pair_q, pair_t, idx1, inlier, node_point_in, n_points, point_status=None, point_xyz=None, max_dist=0.0,
          bridge=1, obs_point_in=None):
    """idx1 / inlier flat (inlier may be None); node_point_in, obs_point_in: lists of N (the latter may be None); point_status:
    list of n_points or None; point_xyz: list of n_points triples or None.  -> dict of lists: point_remap, point_state,
    point_select, node_point, obs_point (None without an input), point_len, totals (6); and for the tests `groups`
    {label: points} and `verdict` {label: state of the group}."""
    N = n_frames * cap
    cls = classes(counts, n_frames, cap, node_point_in, n_points, point_status, bridge)
    groups = groups_of(cls, n_points, point_status, lr.edges(counts, n_frames, cap, pair_q, pair_t, idx1, inlier))
    max2 = float(max_dist) * float(max_dist)
    remap, state, select = list(range(n_points)), [NONE] * n_points, [0] * n_points
    totals, verdict = [0] * 6, {}
    for label in sorted(groups):
        pts = groups[label]
        inside = set(pts)
        frames = [n // cap for n, (c, p) in cls.items() if c == HOLDER and p in inside]
        if len(set(frames)) != len(frames):
            v = CONFLICT
        elif point_xyz is not None and not all(d2(point_xyz[p], point_xyz[label]) <= max2 for p in pts):
            v = FAR
        else:
            v = SURVIVOR
        verdict[label] = v
        for p in pts:
            if v == SURVIVOR:
                remap[p] = label
                state[p] = SURVIVOR if p == label else ABSORBED
            else:
                state[p] = v
        if v == SURVIVOR:
            select[label] = 1
            totals[0] += 1
            totals[1] += len(pts) - 1
        else:
            totals[2 if v == CONFLICT else 3] += 1
            totals[5] += len(pts)

    def rename(v):
        v = int(v)
        return remap[v] if 0 <= v < n_points else v

    node_point = [rename(v) for v in node_point_in[:N]]
    obs_point = None if obs_point_in is None else [rename(v) for v in obs_point_in[:N]]
    point_len = [0] * n_points
    for n in existing(counts, n_frames, cap):
        if 0 <= node_point[n] < n_points:
            point_len[node_point[n]] += 1
        if node_point[n] != int(node_point_in[n]):
            totals[4] += 1
    return dict(point_remap=remap, point_state=state, point_select=select, node_point=node_point, obs_point=obs_point,
                point_len=point_len, totals=totals, groups=groups, verdict=verdict)
