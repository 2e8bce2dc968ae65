"""The track contract of include/gslam_hip.h (gh_triangulate_tracks_dev) restated in scalar IEEE doubles: Python floats,
+ - * / and math.sqrt only, every sum in the stated order.  It shares no code with the library and uses no numpy arithmetic
(BLAS may fuse or reorder); it is the specification the device is held to, bit for bit.  Division and the square root follow
IEEE where Python would raise (x / 0, sqrt of a negative number)."""
import math

OK, TOO_FEW, DEGENERATE, INCONSISTENT, LOW_PARALLAX, SKIPPED = 0, 1, 2, 3, 4, 5
NAN = float("nan")
INF = float("inf")
LANES = 8  # the number of partial sums
DEFAULTS = dict(min_parallax_cos=0.9998, max_reproj=0.004, min_views=2, max_drops=2)
MIN_PIVOT = 1e-12
MIN_DEPTH = 1e-9


def _div(a, b):
    if b != 0.0:
        return a / b
    if a != a or b != b or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if (x >= 0.0 or x != x) else NAN


def quat_rotate(q, p):
    uvx = q[1] * p[2] - q[2] * p[1]
    uvy = q[2] * p[0] - q[0] * p[2]
    uvz = q[0] * p[1] - q[1] * p[0]
    uvx = uvx + uvx
    uvy = uvy + uvy
    uvz = uvz + uvz
    return [(p[0] + q[3] * uvx) + (q[1] * uvz - q[2] * uvy),
            (p[1] + q[3] * uvy) + (q[2] * uvx - q[0] * uvz),
            (p[2] + q[3] * uvz) + (q[0] * uvy - q[1] * uvx)]


def ray(pose, x, y):
    """-> d, the unit ray of (x, y, 1) in the world."""
    w = quat_rotate(pose[:4], (x, y, 1.0))
    s = _div(1.0, _sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
    return [w[0] * s, w[1] * s, w[2] * s]


def normal_terms(d, t):
    """-> [P00 P01 P02 P11 P12 P22 g0 g1 g2] of one observation."""
    P00, P11, P22 = 1.0 - d[0] * d[0], 1.0 - d[1] * d[1], 1.0 - d[2] * d[2]
    P01, P02, P12 = -(d[0] * d[1]), -(d[0] * d[2]), -(d[1] * d[2])
    return [P00, P01, P02, P11, P12, P22,
            (P00 * t[0] + P01 * t[1]) + P02 * t[2],
            (P01 * t[0] + P11 * t[1]) + P12 * t[2],
            (P02 * t[0] + P12 * t[1]) + P22 * t[2]]


def total(terms_by_rank):
    """terms_by_rank: (rank, 9 terms) of the live observations, ascending rank -> the nine sums in the stated order."""
    s = [[0.0] * 9 for _ in range(LANES)]
    for r, v in terms_by_rank:
        part = s[r % LANES]
        for k in range(9):
            part[k] = part[k] + v[k]
    return [((s[0][k] + s[4][k]) + (s[2][k] + s[6][k])) + ((s[1][k] + s[5][k]) + (s[3][k] + s[7][k])) for k in range(9)]


def solve(s):
    """-> X or None (a pivot fails D > 1e-12)."""
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = s
    D0 = A00
    if not (D0 > MIN_PIVOT):
        return None
    L10 = A01 / D0
    L20 = A02 / D0
    D1 = A11 - L10 * A01
    if not (D1 > MIN_PIVOT):
        return None
    u = A12 - L20 * A01
    L21 = u / D1
    D2 = (A22 - L20 * A02) - L21 * u
    if not (D2 > MIN_PIVOT):
        return None
    z0 = b0
    z1 = b1 - L10 * z0
    z2 = (b2 - L20 * z0) - L21 * z1
    y0, y1, y2 = z0 / D0, z1 / D1, z2 / D2
    X2 = y2
    X1 = y1 - L21 * X2
    X0 = (y0 - L10 * X1) - L20 * X2
    return [X0, X1, X2]


def classify(pose, x, y, X, r2):
    """-> (good, drop key)."""
    qc = (-pose[0], -pose[1], -pose[2], pose[3])
    Xc = quat_rotate(qc, (X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]))
    if not (Xc[2] > MIN_DEPTH):
        return False, INF
    iz = 1.0 / Xc[2]
    r0 = Xc[0] * iz - x
    r1 = Xc[1] * iz - y
    e = r0 * r0 + r1 * r1
    return e <= r2, (e if e == e else INF)


def point(obs, **params):
    """One selected point.  obs: its usable observations in track order, each (pose [7], x, y).  -> dict(status, X [3] (zeros
    unless OK), live [bool per rank] (all False unless OK), drops, dropped [ranks in the order they went], anchor (rank of the
    parallax anchor or None))."""
    prm = dict(DEFAULTS, **params)
    need = max(prm["min_views"], 2)
    r2 = prm["max_reproj"] * prm["max_reproj"]
    n = len(obs)
    out = dict(status=TOO_FEW, X=[0.0, 0.0, 0.0], live=[False] * n, drops=0, dropped=[], anchor=None)
    if n < need:
        return out
    obs = [([float(v) for v in pose], float(x), float(y)) for pose, x, y in obs]
    d = [ray(pose, x, y) for pose, x, y in obs]
    terms = [normal_terms(d[r], obs[r][0][4:7]) for r in range(n)]
    live = [True] * n
    nlive = n
    while True:
        X = solve(total([(r, terms[r]) for r in range(n) if live[r]]))
        if X is None:
            out["status"] = DEGENERATE
            return out
        worst, worst_key, all_good = None, -1.0, True
        for r in range(n):
            if live[r]:
                good, key = classify(obs[r][0], obs[r][1], obs[r][2], X, r2)
                all_good = all_good and good
                if key > worst_key:
                    worst, worst_key = r, key
        if all_good:
            break
        if out["drops"] == prm["max_drops"] or nlive == need:
            out["status"] = INCONSISTENT
            return out
        live[worst] = False
        nlive -= 1
        out["drops"] += 1
        out["dropped"].append(worst)
    f = live.index(True)
    out["anchor"] = f
    wide = False
    for k in range(n):
        if live[k] and k != f:
            c = (d[f][0] * d[k][0] + d[f][1] * d[k][1]) + d[f][2] * d[k][2]
            if c < prm["min_parallax_cos"]:
                wide = True
    if not wide:
        out["status"] = LOW_PARALLAX
        return out
    out.update(status=OK, X=X, live=live)
    return out


def tracks(cam_pose, obs_cam, obs_point, obs_xy, n_points, obs_use=None, point_select=None, point_xyz=None, **params):
    """The whole call on host arrays (anything indexable; cam_pose n_cams x 7, obs_xy n_obs x 2; point_xyz: the n_points x 3
    values the array holds on entry, None = zeros).  -> dict of lists: status, n_good, point_xyz per point, obs_good per
    observation, and `results`: the per-point dicts of point() (None for SKIPPED), `tracks`: the observation indices per point."""
    n_cams, n_obs = len(cam_pose), len(obs_cam)
    track = [[] for _ in range(n_points)]
    for i in range(n_obs):
        c, p = int(obs_cam[i]), int(obs_point[i])
        if (obs_use is None or obs_use[i]) and 0 <= c < n_cams and 0 <= p < n_points:
            track[p].append(i)
    res = dict(status=[], n_good=[], point_xyz=[], obs_good=[0] * n_obs, results=[], tracks=track)
    for p in range(n_points):
        if point_select is not None and not point_select[p]:
            res["status"].append(SKIPPED)
            res["n_good"].append(0)
            res["point_xyz"].append([0.0] * 3 if point_xyz is None else [float(v) for v in point_xyz[p]])
            res["results"].append(None)
            continue
        r = point([(cam_pose[int(obs_cam[i])], obs_xy[i][0], obs_xy[i][1]) for i in track[p]], **params)
        res["status"].append(r["status"])
        res["n_good"].append(sum(r["live"]))
        res["point_xyz"].append(r["X"])
        for rank, i in enumerate(track[p]):
            res["obs_good"][i] = 1 if r["live"][rank] else 0
        res["results"].append(r)
    return res
