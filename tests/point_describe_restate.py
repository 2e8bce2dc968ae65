"""The contract of gh_describe_points_dev (include/gslam_hip.h) in plain Python: ints for the bits, Python floats (IEEE doubles,
one rounding per operation) with math.sqrt, the eight partial sums written out.  No numpy in the rules; the device is held to
this byte for byte (tests/test_point_describe_gpu.py), and tests/test_point_describe_cpu.py holds this to a numpy brute force.

describe(...) takes lists: kps_octave N ints, desc N ints of 256 bits (byte i of the descriptor is bits 8 i .. 8 i + 7, which is
int.from_bytes(..., "little")), counts, poses n_frames x 7, the three observation lists, obs_use (list or None), xyz n_points x 3,
status / select (lists or None), and `prev`, the in/out arrays of an earlier call (or None: zeros)."""
import math

OK, EMPTY, NOT_OK, SKIPPED = 0, 1, 2, 3
TRACK_OK = 0
GROUP = 8  # gh_track_group_lanes()
NAN = float("nan")  # CPython's: the quiet NaN 0x7ff8000000000000


def div(a, b):
    """IEEE a / b for b == 0 too (Python raises there)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def canonical(x):
    return NAN if x != x else x


def sqrt(x):
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def power_table(scale_factor, n_levels):
    pw = [1.0]
    for _ in range(1, n_levels):
        pw.append(pw[-1] * scale_factor)
    return pw


def usable_observation(k, counts, n_frames, cap, obs_cam, obs_point, obs_node, obs_use, n_points):
    if obs_use is not None and obs_use[k] == 0:
        return False
    p, n = obs_point[k], obs_node[k]
    if not 0 <= p < n_points or not 0 <= n < n_frames * cap:
        return False
    f, i = n // cap, n % cap
    if not i < min(max(counts[f], 0), cap):
        return False
    return obs_cam[k] == f


def tracks(counts, n_frames, cap, obs_cam, obs_point, obs_node, obs_use, n_points):
    t = [[] for _ in range(n_points)]
    for k in range(len(obs_point)):  # ascending observation index
        if usable_observation(k, counts, n_frames, cap, obs_cam, obs_point, obs_node, obs_use, n_points):
            t[obs_point[k]].append(k)
    return t


def candidates(track, max_views):
    L = len(track)
    M = min(L, max_views)
    if L <= max_views:
        return list(track)
    return [track[(c * L) // M] for c in range(M)]


def medians(cand_desc):
    """med(a) for every candidate: the element at index (M - 1) // 2 of the sorted row of its distances, its own 0 included."""
    M = len(cand_desc)
    out = []
    for a in range(M):
        row = sorted(bin(cand_desc[a] ^ cand_desc[b]).count("1") for b in range(M))
        out.append(row[(M - 1) // 2])
    return out


def choose(cand_desc):
    med = medians(cand_desc)
    best = 0
    for c in range(1, len(med)):
        if med[c] < med[best]:  # strictly: the lowest c wins a tie
            best = c
    return best, med[best]


def unit_ray(X, t):
    v = [X[0] - t[0], X[1] - t[1], X[2] - t[2]]
    r2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    inv = div(1.0, sqrt(r2))
    return [v[0] * inv, v[1] * inv, v[2] * inv], r2


def direction(X, centres):
    """centres: the camera centre of every live observation, in live order -> (normal, r2 of the reference)."""
    s = [[0.0, 0.0, 0.0] for _ in range(GROUP)]
    r2_ref = 0.0
    for i, t in enumerate(centres):
        u, r2 = unit_ray(X, t)
        j = i % GROUP
        for k in range(3):
            s[j][k] = s[j][k] + u[k]
        if i == 0:
            r2_ref = r2
    L = float(len(centres))
    normal = []
    for k in range(3):
        total = ((s[0][k] + s[4][k]) + (s[2][k] + s[6][k])) + ((s[1][k] + s[5][k]) + (s[3][k] + s[7][k]))
        normal.append(canonical(div(total, L)))
    return normal, r2_ref


def describe(kps_octave, desc, counts, n_frames, cap, poses, obs_cam, obs_point, obs_node, obs_use, n_points, xyz, status, select,
             scale_factor=1.2, n_levels=8, max_views=64, prev=None):
    pw = power_table(scale_factor, n_levels)
    if prev is None:
        prev = dict(point_desc=[0] * n_points, point_obs=[[0, 0] for _ in range(n_points)], point_views=[0] * n_points,
                    point_normal=[[0.0, 0.0, 0.0] for _ in range(n_points)], point_dist=[[0.0, 0.0] for _ in range(n_points)])
    out = dict(point_state=[0] * n_points, point_desc=list(prev["point_desc"]), point_obs=[list(v) for v in prev["point_obs"]],
               point_views=list(prev["point_views"]), point_normal=[list(v) for v in prev["point_normal"]],
               point_dist=[list(v) for v in prev["point_dist"]], totals=[0, 0, 0, 0])
    med_of = {}  # not an output: the median of the chosen candidate, for the census
    track = tracks(counts, n_frames, cap, obs_cam, obs_point, obs_node, obs_use, n_points)
    for p in range(n_points):
        if select is not None and select[p] == 0:
            out["point_state"][p] = SKIPPED
            continue
        L = len(track[p])
        if status is not None and status[p] != TRACK_OK:
            state = NOT_OK
        elif L == 0:
            state = EMPTY
        else:
            state = OK
        out["point_state"][p] = state
        if state != OK:
            out["totals"][1 if state == EMPTY else 2] += 1
            out["point_desc"][p] = 0
            out["point_obs"][p] = [-1, -1]
            out["point_views"][p] = 0
            out["point_normal"][p] = [0.0, 0.0, 0.0]
            out["point_dist"][p] = [0.0, 0.0]
            continue
        out["totals"][0] += 1
        if L > max_views:
            out["totals"][3] += 1
        cand = candidates(track[p], max_views)
        best, med_of[p] = choose([desc[obs_node[k]] for k in cand])
        out["point_desc"][p] = desc[obs_node[cand[best]]]
        out["point_obs"][p] = [cand[best], track[p][0]]
        out["point_views"][p] = L
        normal, r2_ref = direction(xyz[p], [poses[obs_node[k] // cap][4:7] for k in track[p]])
        out["point_normal"][p] = normal
        level = min(max(kps_octave[obs_node[track[p][0]]], 0), n_levels - 1)
        max_dist = sqrt(r2_ref) * pw[level]
        min_dist = div(max_dist, pw[n_levels - 1])
        out["point_dist"][p] = [canonical(min_dist), canonical(max_dist)]
    out["med"] = med_of
    out["tracks"] = track
    return out
