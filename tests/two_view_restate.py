"""The two-view contract of include/gslam_hip.h (gh_two_view_batch_dev) restated in scalar IEEE doubles: Python floats,
+ - * / and math.sqrt only, every sum in a stated order.  It shares no code with the library and uses no numpy
arithmetic (BLAS may fuse or reorder); it is the specification the device is held to, bit for bit.  Division and the
square root follow IEEE where Python would raise (x / 0, sqrt of a negative number)."""
import math

OK, NO_MODEL, TOO_FEW, AMBIGUOUS = 0, 1, 2, 3
NAN = float("nan")
INF = float("inf")
DEFAULTS = dict(min_parallax_cos=0.99998, max_reproj=0.004, min_good=50, min_good_permille=900)
# why a row is not good under a candidate (row_rule): 0 = good, else the number of the first test of the contract it fails
GOOD, PARALLEL, BEHIND_RAY, PARALLAX, DEPTH, REPROJ = 0, 1, 2, 3, 4, 5


def _div(a, b):
    if b != 0.0:
        return a / b
    if a != a or b != b or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if (x >= 0.0 or x != x) else NAN


def jacobi3(a):
    """Cyclic Jacobi, twelve sweeps, on the symmetric 3 x 3 `a` (list of lists, destroyed) -> eigenvectors as columns."""
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(12):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = a[p][q]
                if not (abs(apq) > 1e-300):
                    continue
                theta = _div(a[q][q] - a[p][p], 2.0 * apq)
                t = _div(1.0 if theta >= 0 else -1.0, abs(theta) + _sqrt(theta * theta + 1.0))
                c = _div(1.0, _sqrt(t * t + 1.0))
                sn = t * c
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - sn * akq
                    a[k][q] = sn * akp + c * akq
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - sn * aqk
                    a[q][k] = sn * apk + c * aqk
                for k in range(3):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - sn * vkq
                    v[k][q] = sn * vkp + c * vkq
    return v


def decompose(E):
    """E: 9 floats, row-major -> (Ra, Rb, t_hat) as flat lists, or None."""
    E = [float(e) for e in E]
    B = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + E[3 * k + r] * E[3 * k + c]
            B[r][c] = acc
    V = jacobi3(B)
    o = [0, 1, 2]
    for a in range(2):
        for b in range(a + 1, 3):
            if B[o[b]][o[b]] > B[o[a]][o[a]]:
                o[a], o[b] = o[b], o[a]
    l1, l2 = B[o[0]][o[0]], B[o[1]][o[1]]
    if not (l2 > 1e-300):
        return None
    u = [[0.0] * 3 for _ in range(3)]
    v = [[0.0] * 3 for _ in range(3)]
    for a in range(2):
        sv = _sqrt(l1 if a == 0 else l2)
        for r in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + E[3 * r + k] * V[k][o[a]]
            u[a][r] = _div(acc, sv)
            v[a][r] = V[r][o[a]]
    for r in range(3):
        r1, r2 = (r + 1) % 3, (r + 2) % 3
        u[2][r] = u[0][r1] * u[1][r2] - u[0][r2] * u[1][r1]
        v[2][r] = v[0][r1] * v[1][r2] - v[0][r2] * v[1][r1]
    n3 = _sqrt(u[2][0] * u[2][0] + u[2][1] * u[2][1] + u[2][2] * u[2][2])
    if not (n3 > 0.0):
        return None
    th = [_div(u[2][r], n3) for r in range(3)]
    Ra, Rb = [0.0] * 9, [0.0] * 9
    for r in range(3):
        for c in range(3):
            Ra[3 * r + c] = (u[1][r] * v[0][c] - u[0][r] * v[1][c]) + u[2][r] * v[2][c]
            Rb[3 * r + c] = (u[0][r] * v[1][c] - u[1][r] * v[0][c]) + u[2][r] * v[2][c]
    return Ra, Rb, th


def candidates(dec):
    Ra, Rb, th = dec
    tn = [-e for e in th]
    return [(Ra, th), (Ra, tn), (Rb, th), (Rb, tn)]


def row_rule(R, t, x, y, u, v, c2, r2):
    """-> (reason, X_ref): reason GOOD or the first failed test; X_ref is None unless GOOD."""
    b = (u, v, 1.0)
    a = [R[3 * r] * x + R[3 * r + 1] * y + R[3 * r + 2] * 1.0 for r in range(3)]
    aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    at = a[0] * t[0] + a[1] * t[1] + a[2] * t[2]
    bt = b[0] * t[0] + b[1] * t[1] + b[2] * t[2]
    det = aa * bb - ab * ab
    if not (det > 1e-12 * aa * bb):
        return PARALLEL, None
    l1 = _div(ab * bt - bb * at, det)
    l2 = _div(aa * bt - ab * at, det)
    if not (l1 > 0.0) or not (l2 > 0.0):
        return BEHIND_RAY, None
    if ab > 0.0 and ab * ab >= c2 * aa * bb:
        return PARALLAX, None
    mc = [((l1 * a[r] + t[r]) + l2 * b[r]) / 2.0 - t[r] for r in range(3)]
    X = [R[r] * mc[0] + R[3 + r] * mc[1] + R[6 + r] * mc[2] for r in range(3)]
    xc = [(R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]) + t[r] for r in range(3)]
    if not (X[2] > 0.0) or not (xc[2] > 0.0):
        return DEPTH, None
    ex, ey = _div(X[0], X[2]) - x, _div(X[1], X[2]) - y
    fx, fy = _div(xc[0], xc[2]) - u, _div(xc[1], xc[2]) - v
    if not (ex * ex + ey * ey <= r2) or not (fx * fx + fy * fy <= r2):
        return REPROJ, None
    return GOOD, X


def quat(R):
    """Shepperd's largest-pivot rule -> [qx, qy, qz, qw], unit, qw >= 0."""
    tr = R[0] + R[4] + R[8]
    pick, best = 0, tr
    for k, d in ((1, R[0]), (2, R[4]), (3, R[8])):
        if d > best:
            best, pick = d, k
    if pick == 0:
        q = [R[7] - R[5], R[2] - R[6], R[3] - R[1], 1.0 + tr]
    elif pick == 1:
        q = [((1.0 + R[0]) - R[4]) - R[8], R[1] + R[3], R[2] + R[6], R[7] - R[5]]
    elif pick == 2:
        q = [R[1] + R[3], ((1.0 - R[0]) + R[4]) - R[8], R[5] + R[7], R[2] - R[6]]
    else:
        q = [R[2] + R[6], R[5] + R[7], ((1.0 - R[0]) - R[4]) + R[8], R[3] - R[1]]
    n = _sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if q[3] < 0.0:
        q = [-e for e in q]
    return [_div(e, n) for e in q]


def rotation_of(q):
    """(for the checks against ground truth, not part of the contract) rotation matrix of a unit [qx qy qz qw], flat."""
    qx, qy, qz, qw = q
    return [1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
            2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
            2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]


def two_view(E, src, dst, mask=None, **params):
    """One problem.  src, dst: n x 2 (anything indexable), mask: n truthy / falsy or None.  -> dict(status, counts [4],
    n_used, pose [7], points n x [3], good [n], best, reasons n x [4] (None for rows that do not take part))."""
    prm = dict(DEFAULTS, **params)
    c2 = prm["min_parallax_cos"] * prm["min_parallax_cos"]
    r2 = prm["max_reproj"] * prm["max_reproj"]
    n = len(src)
    rows = [(float(src[i][0]), float(src[i][1]), float(dst[i][0]), float(dst[i][1])) for i in range(n)]
    use = [mask is None or bool(mask[i]) for i in range(n)]
    n_used = sum(use)
    dec = decompose(E)
    out = dict(status=NO_MODEL, counts=[0, 0, 0, 0], n_used=n_used, pose=[0.0] * 7, points=[[0.0] * 3 for _ in range(n)],
               good=[0] * n, best=0, reasons=[None] * n)
    if dec is None or n_used == 0:
        return out
    cand = candidates(dec)
    counts = [0, 0, 0, 0]
    for i in range(n):
        if use[i]:
            out["reasons"][i] = [row_rule(R, t, *rows[i], c2, r2)[0] for R, t in cand]
            for k in range(4):
                counts[k] += out["reasons"][i][k] == GOOD
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    out["counts"], out["best"] = counts, best
    if counts[best] < prm["min_good"] or 1000 * counts[best] < prm["min_good_permille"] * n_used:
        out["status"] = TOO_FEW
        return out
    if any(k != best and 10 * counts[k] > 7 * counts[best] for k in range(4)):
        out["status"] = AMBIGUOUS
        return out
    out["status"] = OK
    R, t = cand[best]
    out["pose"] = quat(R) + list(t)
    for i in range(n):
        if use[i]:
            reason, X = row_rule(R, t, *rows[i], c2, r2)
            if reason == GOOD:
                out["points"][i], out["good"][i] = X, 1
    return out


def two_view_batch(E, e_stride, src, dst, offsets, mask=None, fill_point=0.0, fill_good=0, **params):
    """The batch entry on host arrays: E flat (nproblems x e_stride), offsets nproblems + 1 ints.  -> dict of lists: status,
    counts, n_used, poses per problem; points, good per row of src (rows no problem owns keep fill_point / fill_good) and
    `results`, the per-problem dicts of two_view.  A range that is empty, reversed or outside 0 .. offsets[-1] is 0 rows."""
    npb = len(offsets) - 1
    limit = int(offsets[npb])
    total = len(src)
    res = dict(status=[], counts=[], n_used=[], poses=[], points=[[fill_point] * 3 for _ in range(total)],
               good=[fill_good] * total, results=[])
    for p in range(npb):
        b, e = int(offsets[p]), int(offsets[p + 1])
        if b < 0 or e > limit or e <= b:
            b = e = 0
        r = two_view([E[p * e_stride + k] for k in range(9)], src[b:e], dst[b:e], None if mask is None else mask[b:e], **params)
        res["status"].append(r["status"])
        res["counts"].append(r["counts"])
        res["n_used"].append(r["n_used"])
        res["poses"].append(r["pose"])
        res["points"][b:e] = r["points"]
        res["good"][b:e] = r["good"]
        res["results"].append(r)
    return res
