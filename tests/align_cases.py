"""A deterministic census of 3-D alignment problems (gh_align_sim3 / oracle_align_sim3: dst ~ s R src + t) at the places
where a closed-form Horn fit goes wrong: the block boundaries of the 256-wide fold, clouds far from the origin (a
trajectory in GPS coordinates), extreme scales, the dof masks, a rotation of exactly pi, a mirrored cloud, coplanar and
collinear clouds, src == dst, and the degenerate sets that must be refused.

Each case is (name, src n x 3, dst n x 3, dof, truth) with truth = the generating [qx qy qz qw tx ty tz s] where the
case is noise-free and the fit is unique, else None (the reference is then a high-precision centred Horn fit).
expect_refused(name) and rotation_is_free(name) tell the two kinds of case that are not compared transform to transform.

Shared by tests/test_align_adversarial_oracle.py (CPU) and tests/test_align_adversarial_gpu.py; plain numpy, float64."""
import numpy as np

from gslam_amd.pg_synth import _qrot

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
NOISE = 0.02


def rotmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def apply(S, pts):
    """S * p = R (s p) + t, with the oracle's own rotation formula and order of operations."""
    q = np.asarray(S[:4], np.float64)
    u = 2.0 * np.cross(q[None, :3], pts)
    Ra = pts + q[3] * u + np.cross(q[None, :3], u)
    return S[7] * Ra + S[4:7]


def expect_refused(name):
    return name.startswith("refused_")


def rotation_is_free(name):
    return name.startswith("collinear")


def _unit(rng, k=3):
    v = rng.normal(size=k)
    return v / np.linalg.norm(v)


def _transform(rng, scale=None, quat=None):
    q = _unit(rng, 4) if quat is None else np.asarray(quat, np.float64)
    if q[3] < 0:
        q = -q
    s = float(np.exp(rng.uniform(-0.4, 0.4))) if scale is None else float(scale)
    return q, s


def _make(rng, local, q, s, off_a, off_b, noise=0.0, mirror=False):
    """src = off_a + local, dst = off_b + s R local (+ noise): both clouds are formed from the LOCAL coordinates, so the
    generating transform (q, off_b - s R off_a, s) is the truth to the rounding of the stored coordinates."""
    loc = local * np.array([1.0, 1.0, -1.0]) if mirror else local
    src = off_a + local
    dst = off_b + s * np.stack([_qrot(q, p) for p in loc])
    if noise > 0:
        dst = dst + rng.normal(size=dst.shape) * noise
    truth = np.concatenate([q, off_b - s * _qrot(q, off_a), [s]])
    return src, dst, truth


def build():
    cases = []
    zero = np.zeros(3)

    # the block boundaries of the 256-wide fold
    for n in (3, 4, 255, 256, 257, 513):
        rng = np.random.default_rng(1000 + n)
        q, s = _transform(rng)
        src, dst, truth = _make(rng, rng.normal(size=(n, 3)) * 4, q, s, rng.normal(size=3), rng.normal(size=3) * 3)
        cases.append(("n%d" % n, src, dst, 127, truth))

    # far from the origin, different offsets on the two clouds, noise-free and noisy
    for off in (0.0, 1e3, 1e5, 4e6):
        for spread in (10.0, 1.0):
            for noise in (0.0, NOISE):
                rng = np.random.default_rng(int(2000 + np.log10(off + 1) * 10 + spread))
                q, s = _transform(rng, scale=1.3)
                local = rng.normal(size=(1000, 3)) * spread
                off_a, off_b = off * _unit(rng), 0.7 * off * _unit(rng)
                src, dst, truth = _make(rng, local, q, s, off_a, off_b, noise=noise)
                tag = {0.0: "0", 1e3: "1e3", 1e5: "1e5", 4e6: "4e6"}[off]
                cases.append(("offset%s_spread%g_%s" % (tag, spread, "noisy" if noise else "exact"), src, dst, 127,
                              None if noise else truth))

    # extreme scales
    for s in (1e-6, 1e6):
        rng = np.random.default_rng(31)
        q, _ = _transform(rng)
        src, dst, truth = _make(rng, rng.normal(size=(300, 3)) * 5, q, s, np.array([3.0, -2.0, 1.0]), np.array([-1.0, 4.0, 2.0]))
        cases.append(("scale%g" % s, src, dst, 127, truth))

    # dof masks: no scale bit (rotation + translation, translation only -- the closed form looks at GH_KF_SCALE alone),
    # scale with translation only, and no scale bit on data that does carry a scale (no exact truth then)
    for name, dof, s, exact in (("dof63", 63, 1.0, True), ("dof7", 7, 1.0, True), ("dof7_scale", 7 | 64, 0.8, True),
                                ("dof63_on_scaled_data", 63, 1.25, False)):
        rng = np.random.default_rng(41 + dof)
        q, _ = _transform(rng)
        src, dst, truth = _make(rng, rng.normal(size=(200, 3)) * 3, q, s, np.array([1.0, 2.0, 3.0]), np.array([0.5, -0.5, 2.0]),
                                noise=0.0 if exact else NOISE)
        cases.append((name, src, dst, dof, truth if exact else None))

    # a rotation of exactly pi: qw = 0, the sign of the quaternion is free
    rng = np.random.default_rng(51)
    axis = _unit(rng)
    src, dst, truth = _make(rng, rng.normal(size=(100, 3)) * 2, np.concatenate([axis, [0.0]]), 1.1, zero + 1.0, zero - 2.0)
    cases.append(("rotation_pi", src, dst, 127, truth))
    src, dst, truth = _make(rng, rng.normal(size=(100, 3)) * 2, np.array([0.0, 0.0, 1.0, 0.0]), 1.0, zero, zero)
    cases.append(("rotation_pi_about_z", src, dst, 127, truth))

    # a mirrored dst: the best PROPER rotation (Umeyama with the determinant fix), no exact truth
    rng = np.random.default_rng(61)
    q, s = _transform(rng)
    src, dst, _ = _make(rng, rng.normal(size=(150, 3)) * np.array([4.0, 2.0, 1.0]), q, s, zero + 2.0, zero - 1.0, mirror=True)
    cases.append(("mirrored", src, dst, 127, None))

    # coplanar (the fit is still unique) and collinear (the rotation about the line is free)
    rng = np.random.default_rng(71)
    q, s = _transform(rng)
    local = rng.normal(size=(120, 3)) * 3
    local[:, 2] = 0.0
    src, dst, truth = _make(rng, local, q, s, np.array([5.0, 1.0, -2.0]), np.array([0.0, 3.0, 3.0]))
    cases.append(("coplanar", src, dst, 127, truth))
    src, dst, _ = _make(rng, local, q, s, np.array([5.0, 1.0, -2.0]), np.array([0.0, 3.0, 3.0]), noise=NOISE)
    cases.append(("coplanar_noisy", src, dst, 127, None))
    for name, off in (("collinear", 0.0), ("collinear_offset1e5", 1e5)):
        rng = np.random.default_rng(81)
        q, s = _transform(rng)
        local = np.outer(rng.normal(size=90) * 4, _unit(rng))
        src, dst, _ = _make(rng, local, q, s, off * _unit(rng) + 1.0, 0.7 * off * _unit(rng) - 1.0)
        cases.append((name, src, dst, 127, None))

    # src == dst, at the origin and far from it
    rng = np.random.default_rng(91)
    pts = rng.normal(size=(260, 3)) * 2
    cases.append(("same_cloud", pts, pts.copy(), 127, IDENTITY.copy()))
    far = pts + np.array([4e6, -1e6, 2e5])
    cases.append(("same_cloud_offset4e6", far, far.copy(), 127, IDENTITY.copy()))

    # refused: all points coincident (one cloud, the other, both; also away from the origin, where raw sums would leave
    # rounding noise in place of a zero spread), and fewer than three correspondences
    one = np.tile(np.array([1234.5, -0.1, 7e5]), (10, 1))
    cases.append(("refused_src_coincident", one, rng.normal(size=(10, 3)), 127, None))
    cases.append(("refused_dst_coincident", rng.normal(size=(10, 3)), one, 127, None))
    cases.append(("refused_both_coincident", one, one[:, ::-1].copy(), 127, None))
    cases.append(("refused_n2", rng.normal(size=(2, 3)), rng.normal(size=(2, 3)), 127, None))
    cases.append(("refused_n1", rng.normal(size=(1, 3)), rng.normal(size=(1, 3)), 127, None))
    cases.append(("refused_n0", np.zeros((0, 3)), np.zeros((0, 3)), 127, None))
    return [(name, np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64), dof, truth)
            for name, a, b, dof, truth in cases]


CASES = build()
NAMES = [c[0] for c in CASES]


def horn_centred(src, dst, with_scale):
    """The plain float64 reference: two-pass centred Horn (centroids first, then the moments of the centred clouds, then
    the largest eigenvector of the 4 x 4 N matrix by numpy's eigh)."""
    ca, cb = src.mean(0), dst.mean(0)
    A, B = src - ca, dst - cb
    M = A.T @ B
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    qw, qx, qy, qz = V[:, 3] * (1.0 if V[0, 3] >= 0 else -1.0)
    q = np.array([qx, qy, qz, qw])
    s = float(np.sqrt((B * B).sum() / (A * A).sum())) if with_scale else 1.0
    return np.concatenate([q, cb - s * rotmat(q) @ ca, [s]])


def errors(S, ref, dst):
    """The three measures: rotation max |R - R*| (free of the sign of the quaternion), scale relative, translation
    relative to max(1, |centroid of dst|)."""
    c = max(1.0, float(np.linalg.norm(dst.mean(0))))
    return (float(np.abs(rotmat(S[:4]) - rotmat(ref[:4])).max()), abs(S[7] - ref[7]) / ref[7],
            float(np.abs(S[4:7] - ref[4:7]).max()) / c)


def image_error(S, src, dst_ref):
    """Where the rotation is not unique: the image of the points, relative to max(1, |centroid of dst|)."""
    c = max(1.0, float(np.linalg.norm(dst_ref.mean(0))))
    return float(np.abs(apply(S, src) - dst_ref).max()) / c


def header_expressions(S, src, dst, dof, sequential):
    """ssq and the 7 x 7 information as include/gslam_hip.h defines them, at the transform S: r_k = dst_k - S src_k and
    J^T J = s^2 sum D_k^T D_k with D_k = [I | -[a]x | a] of the UNCENTRED a = src_k, masked by dof.  The residuals are
    formed in numpy's long double (coordinates of 4e6 m leave 5e-10 m of rounding per point in float64, more than the
    bars on ssq allow), the information in float64 with the per-point terms in the oracle's order of operations.  The
    per-point terms are the same in both summation orders: sequential (cumsum) or numpy's pairwise sum."""
    total = (lambda v: np.cumsum(v)[-1]) if sequential else (lambda v: np.sum(v))
    L = np.longdouble
    x, y, z, w = (L(v) for v in S[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=L) / (x * x + y * y + z * z + w * w)
    r = dst.astype(L) - (L(S[7]) * (src.astype(L) @ R.T) + S[4:7].astype(L))
    ssq = float(total((r * r).reshape(-1)))
    n = len(src)
    a = src
    o, z = np.ones(n), np.zeros(n)
    D = np.array([[o, z, z, z, a[:, 2], -a[:, 1], a[:, 0]], [z, o, z, -a[:, 2], z, a[:, 0], a[:, 1]],
                  [z, z, o, a[:, 1], -a[:, 0], z, a[:, 2]]])
    info = np.zeros((7, 7))
    for p in range(7):
        for c in range(7):
            if (dof >> p) & 1 and (dof >> c) & 1:
                info[p, c] = float(total((S[7] * S[7]) * ((D[0, p] * D[0, c] + D[1, p] * D[1, c]) + D[2, p] * D[2, c])))
    return ssq, info


def ssq_margin(S, src, dst, ssq, order_difference):
    """How far a correct ssq may be from header_expressions': 10 x the difference between the two summation orders, one
    rounding of the value, the rounding of the long-double residuals (each exact to eps_L * D, D = the largest
    coordinate: 4 sqrt(n ssq) eps_L D on the sum), the rounding of float64 residuals taken about the first
    correspondence (each exact to eps * Dp, Dp = the largest coordinate about that pivot: 4 sqrt(n ssq) eps Dp, and
    n (4 eps Dp)^2 where the fit is exact), and the rounding of the returned translation: t is exact to a few
    ulp of D, and moving t by d changes the sum by n d^2 + 2 d . (sum of the residuals), whose second term vanishes at
    the fit: n (4 eps D)^2."""
    eps, eps_l = 2.220446049250313e-16, float(np.finfo(np.longdouble).eps)
    n = len(src)
    D = max(float(np.abs(dst).max()), float(S[7] * np.abs(src).max()))
    Dp = max(float(np.abs(dst - dst[0]).max()), float(S[7] * np.abs(src - src[0]).max()))
    return (10.0 * abs(order_difference) + 4 * eps * ssq + 4.0 * np.sqrt(n * ssq) * (eps_l * D + eps * Dp) + n * (4 * eps * D) ** 2
            + n * (4 * eps * Dp) ** 2)
