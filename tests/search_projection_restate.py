"""The contract of gh_search_projection_dev (include/gslam_hip.h) in plain Python: ints, floats (IEEE doubles) and math.sqrt, no
numpy in the arithmetic.  Every operation is written in the order the contract fixes; Python rounds each once and fuses nothing.
The keypoint coordinates come in as Python floats that hold the float32 values exactly (the widening of the contract).
search(...) returns the outputs and the verdict of every (searched frame, searchable point) pair."""
import math

HELD, BEHIND, OUTSIDE, RANGE, ANGLE, NO_CANDIDATE, WEAK, RATIO, LOST, WON = range(10)
VERDICTS = ("HELD", "BEHIND", "OUTSIDE", "RANGE", "ANGLE", "NO_CANDIDATE", "WEAK", "RATIO", "LOST", "WON")
TRACK_OK = 0
LOC_NO_POINT, LOC_NO_ROW = -1, -3
NO_DIST = 0xFFFF
MIN_DEPTH = 1e-9
DEFAULTS = dict(scale_factor=1.2, radius_near=2.5, radius_far=4.0, near_cos=0.998, radius_scale=1.0, min_view_cos=0.5, range_lo=0.8,
                range_hi=1.2, nn_ratio=0.8, n_levels=8, max_hamming=100)
# the near rules of tests/test_search_projection_cpu.py: each must change an output on the cases
RULES = ("closed_window", "log_level", "highest_row")


def quat_rotate(q, p):
    """gh_ba::quat_rotate, the formula under gh_triangulate_tracks_dev."""
    uvx, uvy, uvz = q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]
    uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
    return [p[0] + q[3] * uvx + (q[1] * uvz - q[2] * uvy),
            p[1] + q[3] * uvy + (q[2] * uvx - q[0] * uvz),
            p[2] + q[3] * uvz + (q[0] * uvy - q[1] * uvx)]


def pow_table(scale_factor, n=32):
    t = [1.0]
    for _ in range(1, n):
        t.append(t[-1] * scale_factor)
    return t


def _div(a, b):
    """IEEE division: Python raises where the hardware gives an infinity or a NaN."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.nan if x != x or x < 0.0 else math.sqrt(x)


def project(pose, X, fx, fy, cx, cy):
    """-> d, Xc and (u, v) (None when the point is not in front)."""
    d = [X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]]
    Xc = quat_rotate([-pose[0], -pose[1], -pose[2], pose[3]], d)
    if not Xc[2] > MIN_DEPTH:
        return d, Xc, None
    iz = _div(1.0, Xc[2])
    return d, Xc, (fx * (Xc[0] * iz) + cx, fy * (Xc[1] * iz) + cy)


def search(kps_x, kps_y, kps_octave, desc, counts, n_frames, cap, poses, frame_search, node_point_in, row_point_in, row_inlier_in,
           n_points, xyz, status, select, views, point_desc, normal, dist, fx, fy, cx, cy, width, height, params, rule=None):
    """kps_x / kps_y / kps_octave, desc (256-bit ints): n_frames * cap entries; node_point_in, row_point_in + row_inlier_in, status,
    select: lists or None; point_desc: 256-bit ints; normal n_points x 3, dist n_points x 2; params: a dict as DEFAULTS.
    rule: None (the contract) or one of RULES (a near rule, for the tests that show the cases tell them apart).
    -> dict: row_point, row_inlier, row_dist (N each), frame_totals (n_frames x 10), totals (12), verdict {(f, p): code},
    detail {(f, p): dict of what the pair computed}."""
    N = n_frames * cap
    out = dict(row_point=None, row_inlier=None, row_dist=None, frame_totals=None, totals=[0] * 12, verdict={}, detail={})
    if N == 0:
        return out
    pw = pow_table(params["scale_factor"])
    rows = [min(max(c, 0), cap) for c in counts]
    claims = row_point_in is not None
    exists = [n % cap < rows[n // cap] for n in range(N)]
    taken = [-1] * N
    for n in range(N):
        if not exists[n]:
            continue
        if node_point_in is not None and 0 <= node_point_in[n] < n_points:
            taken[n] = node_point_in[n]
        elif claims and row_inlier_in[n] != 0 and 0 <= row_point_in[n] < n_points:
            taken[n] = row_point_in[n]
    searched = [f for f in range(n_frames) if frame_search[f] != 0]
    searchable = [p for p in range(n_points) if (select is None or select[p] != 0) and (status is None or status[p] == TRACK_OK)
                  and views[p] > 0]
    ft = [[0] * 10 for _ in range(n_frames)]
    proposals = {}  # node -> list of (h, p)
    for f in searched:
        held = set(taken[n] for n in range(f * cap, f * cap + rows[f]) if taken[n] >= 0)
        open_rows = [i for i in range(rows[f]) if taken[f * cap + i] < 0]
        for p in searchable:
            det = {}
            out["detail"][(f, p)] = det
            v = _pair(f, p, det, held, open_rows, kps_x, kps_y, kps_octave, desc, cap, poses[f], xyz[p], point_desc[p], normal[p],
                      dist[p], fx, fy, cx, cy, width, height, params, pw, rule)
            out["verdict"][(f, p)] = v
            if v is None:
                proposals.setdefault(f * cap + det["best"], []).append((det["h_best"], p))
            else:
                ft[f][v] += 1
    won = {}
    for n, props in proposals.items():
        h, p = min(props)
        won[n] = (h, p)
        for hh, pp in props:
            v = WON if (hh, pp) == (h, p) else LOST
            out["verdict"][(n // cap, pp)] = v
            ft[n // cap][v] += 1
    row_point, row_inlier, row_dist = [0] * N, [0] * N, [NO_DIST] * N
    for n in range(N):
        if n in won:
            row_point[n], row_inlier[n], row_dist[n] = won[n][1], 1, won[n][0]
        elif claims:
            row_point[n], row_inlier[n] = row_point_in[n], 1 if row_inlier_in[n] != 0 else 0
        else:
            row_point[n] = LOC_NO_POINT if exists[n] else LOC_NO_ROW
    totals = [sum(ft[f][k] for f in range(n_frames)) for k in range(10)]
    totals += [len(searched), len(searchable) if searched else 0]  # (no searched frame: every count is zero)
    out.update(row_point=row_point, row_inlier=row_inlier, row_dist=row_dist, frame_totals=ft, totals=totals)
    return out


def _pair(f, p, det, held, open_rows, kps_x, kps_y, kps_octave, desc, cap, pose, X, pdesc, nrm, pdist, fx, fy, cx, cy, width, height,
          prm, pw, rule):
    """The verdict of one pair, or None when it proposes (det then says to whom)."""
    if p in held:
        return HELD
    d, Xc, uv = project(pose, X, fx, fy, cx, cy)
    if uv is None:
        return BEHIND
    u, v = uv
    det["u"], det["v"] = u, v
    if not (0.0 <= u and u < float(width) and 0.0 <= v and v < float(height)):
        return OUTSIDE
    r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    dd = _sqrt(r2)
    det["dist"] = dd
    min_dist, max_dist = pdist
    if not (dd >= prm["range_lo"] * min_dist and dd <= prm["range_hi"] * max_dist):
        return RANGE
    c = _div((d[0] * nrm[0] + d[1] * nrm[1]) + d[2] * nrm[2], dd)
    det["cos"] = c
    if not c >= prm["min_view_cos"]:
        return ANGLE
    level = sum(1 for l in range(0, prm["n_levels"] - 1) if pw[l] * dd < max_dist)
    if rule == "log_level":  # ORB-SLAM's own words
        ratio = max_dist / dd
        level = int(math.ceil(math.log(ratio) / math.log(prm["scale_factor"]))) if prm["scale_factor"] > 1.0 and ratio > 0.0 else 0
        level = min(max(level, 0), prm["n_levels"] - 1)
    radius = (prm["radius_scale"] * (prm["radius_near"] if c > prm["near_cos"] else prm["radius_far"])) * pw[level]
    det["level"], det["radius"] = level, radius
    cand = []
    for i in open_rows:
        n = f * cap + i
        if not (level - 1 <= kps_octave[n] <= level):
            continue
        ax, ay = abs(kps_x[n] - u), abs(kps_y[n] - v)
        inside = (ax <= radius and ay <= radius) if rule == "closed_window" else (ax < radius and ay < radius)
        if inside:
            cand.append(((pdesc ^ desc[n]).bit_count(), i))
    det["candidates"] = [i for _, i in cand]
    if not cand:
        return NO_CANDIDATE
    cand.sort(key=(lambda k: (k[0], -k[1])) if rule == "highest_row" else None)
    h_best, best = cand[0]
    h_second, oct_second = (cand[1][0], kps_octave[f * cap + cand[1][1]]) if len(cand) > 1 else (256, -1)
    det["h_best"], det["best"], det["h_second"] = h_best, best, h_second
    if h_best > prm["max_hamming"]:
        return WEAK
    if kps_octave[f * cap + best] == oct_second and float(h_best) > prm["nn_ratio"] * float(h_second):
        return RATIO
    return None
