"""The alignment oracle (oracle_align_sim3, oracle/pg_oracle.c) against references that share no formula with it, on
the census of tests/align_cases.py.  The GPU kernel is held to the oracle in tests/test_align_adversarial_gpu.py, and the
two share their formula (sums, then Horn's closed form), so this file is what pins the formula itself.

Reference: the generating transform where the case is noise-free and the fit unique; otherwise a centred Horn fit in
mpmath at 60 digits (mpmath.eigsy for the 4 x 4 eigenproblem), and for the mirrored cloud Umeyama's SVD form with the
determinant fix, also in mpmath.  Measures: rotation max |R - R*|, scale relative, translation relative to
max(1, |centroid of dst|); where the rotation about a line is free (collinear clouds), the image of the points instead.

Bar, per case and per measure: max(16 * e_c, 1e-11), e_c = the error of a float64 two-pass centred Horn in numpy
(align_cases.horn_centred) against the same reference.  1e-11 is the bar test_alignment_parity holds at the origin; 16 is
one bit of slack per power of two of n in the fold (n <= 1000 < 2^10 would even allow more) and well above the 2-3x seen
between summation orders.  Measured on this census (test_oracle_meets_the_reference prints every case):
    worst e_c          rotation 3.3e-12  scale 3.8e-12  translation 7.5e-12    (offset 4e6 m, spread 1 m, noise-free)
    worst oracle error rotation 3.3e-12  scale 3.8e-12  translation 7.4e-12    (the same case: 1.0 x its e_c)
    (that is the rounding of the stored coordinates, ulp(4e6) = 5e-10 m on a cloud 1 m across, not of either fit;)
    everywhere else both are below 2e-12, and where e_c is a few 1e-16 the oracle is at most 9e-14
    worst image error on the collinear clouds: oracle 1.4e-15, numpy 1.4e-15

Before the moments were taken about a pivot (raw sums sum a, sum a b^T, sum |a|^2 and "- n ca cb^T" afterwards) this test
fails on 14 cases: every cloud 1e5 m or further from the origin, and already at 1e3 m with a spread of 1 m.  The oracle
of the parent commit measured, noise-free, true scale 1.3 (bars: 1e-11, at offset 4e6 / spread 1 m 5e-11 .. 1e-10):
    offset 1e3, spread 1 m    rotation 2.2e-10   scale 8.8e-11   translation 5.3e-10
    offset 1e5, spread 10 m   rotation 3.8e-08   scale 4.7e-09   translation 6.3e-08
    offset 1e5, spread 1 m    rotation 1.8e-06   scale 3.0e-06   translation 6.7e-06
    offset 4e6, spread 10 m   rotation 1.1e-05   scale 6.1e-06   translation 2.6e-05
    offset 4e6, spread 1 m    rotation 3.2e-03   scale 5.8e-03   translation 1.0e-02
and the same against the 60-digit fit with 0.02 m noise; scale1e-06 (a dst cloud 5e-6 across, 4.6 from the origin) had a
scale error of 2.4e-05, same_cloud_offset4e6 a rotation 1.7e-05 off the identity.  The refused sets came back with an
all-zero quaternion where gh_align_sim3 writes the identity; the oracle writes the identity now.

ssq and the information matrix are compared with align_cases.header_expressions: a numpy evaluation of the expressions
of include/gslam_hip.h at the transform the oracle returned -- the residuals dst - S src in long double, the information
in float64 with the per-point terms in the oracle's order of operations.  The margin is 10 x the difference between two
summation orders of that evaluation (sequential against numpy's pairwise), per case and per entry, plus the roundings
that separate two correct evaluations (align_cases.ssq_margin writes each term down; for the information one rounding
of the value, 4 * 2.2e-16 relative, which is all that is left when the two orders agree to the bit, as for n < 8).
Measured: the largest margin is 5.0e-11 relative (ssq of offset4e6_spread10_noisy, from the long-double rounding of
coordinates of 4e6 m) and 2.5e-13 absolute on the ssq of the noise-free cases; the oracle uses at most 0.29 of it (0.00
on the information: its order is the sequential one).  With the residuals formed in float64 from the uncentred
coordinates, as before this change, the oracle and the kernel were 1.7e-9 apart on that ssq of 1.23 -- fourteen times
the 1e-10 that tests/test_align_adversarial_gpu.py allows -- and 30 x this margin; the residuals are now taken about the
same pivot as the moments."""
import numpy as np
import pytest

import align_cases as ac

mp = pytest.importorskip("mpmath")

EPS = 2.220446049250313e-16
FLOOR = 1e-11
SLACK = 16.0


def _mp_rot(q):
    x, y, z, w = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _mp_fit(src, dst, with_scale, umeyama=False):
    """Centred Horn (or Umeyama's SVD with the determinant fix) at 60 digits -> float64 [q t s]."""
    with mp.workdps(60):
        n = len(src)
        A = [[mp.mpf(float(v)) for v in p] for p in src]
        B = [[mp.mpf(float(v)) for v in p] for p in dst]
        ca = [mp.fsum(p[e] for p in A) / n for e in range(3)]
        cb = [mp.fsum(p[e] for p in B) / n for e in range(3)]
        A = [[p[e] - ca[e] for e in range(3)] for p in A]
        B = [[p[e] - cb[e] for e in range(3)] for p in B]
        M = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                M[r, c] = mp.fsum(A[k][r] * B[k][c] for k in range(n))
        na = mp.fsum(v * v for p in A for v in p)
        nb = mp.fsum(v * v for p in B for v in p)
        if umeyama:
            U, D, Vt = mp.svd_r(M.T)  # M^T = sum b a^T = U D V^T, R = U diag(1, 1, det(U V^T)) V^T
            W = mp.diag([1, 1, mp.sign(mp.det(U) * mp.det(Vt))])
            R = U * W * Vt
        else:
            N = mp.matrix([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                           [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                           [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                           [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
            for r in range(1, 4):
                for c in range(r):
                    N[r, c] = N[c, r]
            E, Q = mp.eigsy(N)
            best = max(range(4), key=lambda k: E[k])
            qw, qx, qy, qz = (Q[k, best] for k in range(4))
            R = _mp_rot((qx, qy, qz, qw))
        s = mp.sqrt(nb / na) if with_scale else mp.mpf(1)
        t = mp.matrix(cb) - s * (R * mp.matrix(ca))
        return np.array([[float(R[r, c]) for c in range(3)] for r in range(3)]), np.array([float(v) for v in t]), float(s)


def _errors_R(S, R, t, s, dst):
    c = max(1.0, float(np.linalg.norm(dst.mean(0))))
    return (float(np.abs(ac.rotmat(S[:4]) - R).max()), abs(S[7] - s) / s, float(np.abs(S[4:7] - t).max()) / c)


@pytest.fixture(scope="module")
def references():
    """name -> (R, t, s) of the reference, computed once."""
    out = {}
    for name, src, dst, dof, truth in ac.CASES:
        if ac.expect_refused(name) or ac.rotation_is_free(name):
            continue
        if truth is not None:
            out[name] = (ac.rotmat(truth[:4]), truth[4:7], truth[7])
        else:
            out[name] = _mp_fit(src, dst, bool(dof & 64), umeyama=name == "mirrored")
    return out


def test_census_is_what_it_says():
    names = set(ac.NAMES)
    assert len(names) == len(ac.CASES)
    for n in (3, 4, 255, 256, 257, 513):
        assert "n%d" % n in names
    for name, src, dst, dof, truth in ac.CASES:
        assert src.shape == dst.shape and src.dtype == dst.dtype == np.float64
        if name.startswith("offset4e6"):
            assert np.linalg.norm(src.mean(0)) > 3e6 and np.linalg.norm(dst.mean(0)) > 2e6
            assert np.linalg.norm(src.mean(0) - dst.mean(0)) > 1e5  # different offsets on the two clouds
    S = dict((c[0], c) for c in ac.CASES)
    assert S["rotation_pi"][4][3] == 0.0 and np.linalg.matrix_rank(S["coplanar"][1] - S["coplanar"][1].mean(0)) == 2
    assert np.linalg.matrix_rank(S["collinear"][1] - S["collinear"][1].mean(0), tol=1e-9) == 1
    assert not any(dof & 64 for name, _, _, dof, _ in ac.CASES if name in ("dof63", "dof7", "dof63_on_scaled_data"))


def test_mirrored_reference_is_the_best_proper_rotation(references):
    """Horn's largest eigenvector and Umeyama's determinant fix are the same maximiser of tr(R^T M) over SO(3): the two
    60-digit routes agree, and the mirror image itself (det = -1) is not what either returns."""
    name, src, dst, dof, _ = next(c for c in ac.CASES if c[0] == "mirrored")
    R, t, s = references[name]
    Rh, th, sh = _mp_fit(src, dst, True, umeyama=False)
    assert np.abs(R - Rh).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(t - th).max() < 1e-13 and s == sh


def test_oracle_meets_the_reference(oracle, references):
    worst_c, worst_o, worst_img, bad = np.zeros(3), np.zeros(3), np.zeros(2), []
    for name, src, dst, dof, truth in ac.CASES:
        ok, S, _, _ = oracle.align_sim3(src, dst, dof)
        if ac.expect_refused(name):
            assert not ok and S.tolist() == ac.IDENTITY.tolist(), name
            continue
        assert ok, name
        Sc = ac.horn_centred(src, dst, bool(dof & 64))
        if ac.rotation_is_free(name):
            e_c, e_o = ac.image_error(Sc, src, dst), ac.image_error(S, src, dst)
            worst_img = np.maximum(worst_img, [e_c, e_o])
            print("%-28s image error: numpy %.1e  oracle %.1e" % (name, e_c, e_o))
            if e_o > max(SLACK * e_c, FLOOR):
                bad.append((name, "image", e_o, e_c))
            continue
        e_c = np.array(_errors_R(Sc, *references[name], dst))
        e_o = np.array(_errors_R(S, *references[name], dst))
        worst_c, worst_o = np.maximum(worst_c, e_c), np.maximum(worst_o, e_o)
        print("%-28s e_c rot %.1e scale %.1e trans %.1e | oracle rot %.1e scale %.1e trans %.1e" % ((name,) + tuple(e_c) + tuple(e_o)))
        for k, what in enumerate(("rotation", "scale", "translation")):
            if e_o[k] > max(SLACK * e_c[k], FLOOR):
                bad.append((name, what, e_o[k], e_c[k]))
        if not dof & 64:
            assert S[7] == 1.0, name
        assert S[3] >= 0.0 and abs(np.linalg.norm(S[:4]) - 1.0) < 4 * EPS, name
    print("worst e_c (rot, scale, trans) %s; worst oracle error %s; collinear image error numpy %.1e oracle %.1e"
          % (worst_c, worst_o, worst_img[0], worst_img[1]))
    assert not bad, bad


def test_oracle_ssq_and_information_are_the_header_expressions(oracle):
    worst_margin, worst_ratio, worst_abs = 0.0, 0.0, 0.0
    for name, src, dst, dof, truth in ac.CASES:
        if ac.expect_refused(name):
            continue
        ok, S, info, ssq = oracle.align_sim3(src, dst, dof)
        ssq1, info1 = ac.header_expressions(S, src, dst, dof, sequential=True)
        ssq2, info2 = ac.header_expressions(S, src, dst, dof, sequential=False)
        m_ssq = ac.ssq_margin(S, src, dst, ssq1, ssq1 - ssq2)
        m_info = 10.0 * np.abs(info1 - info2) + 4 * EPS * np.abs(info1)
        assert abs(ssq - ssq1) <= m_ssq, (name, ssq, ssq1, m_ssq)
        assert (np.abs(info - info1) <= m_info).all(), (name, np.abs(info - info1).max())
        on = np.array([(dof >> k) & 1 for k in range(7)], bool)
        assert not info[~on].any() and not info[:, ~on].any() and np.array_equal(info, info.T), name
        rel = max(m_ssq / ssq1 if ssq1 > 1e-6 else 0.0, float((m_info[info1 != 0] / np.abs(info1[info1 != 0])).max()))
        if ssq1 <= 1e-6:
            worst_abs = max(worst_abs, m_ssq)
        worst_margin = max(worst_margin, rel)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.nanmax(np.append((np.abs(info - info1) / m_info)[m_info > 0], abs(ssq - ssq1) / m_ssq if m_ssq > 0 else 0.0))
        worst_ratio = max(worst_ratio, float(ratio))
    print("largest margin: %.1e relative (noisy cases, information entries), %.1e absolute (ssq of the exact cases); the oracle uses "
          "at most %.2f of its margin" % (worst_margin, worst_abs, worst_ratio))


def test_translation_invariance(oracle):
    """The property itself: moving both clouds (by different, exactly representable vectors) changes R and s by rounding
    only, and t by what the move implies.  Power-of-two shifts of an integer-valued cloud are exact in float64."""
    rng = np.random.default_rng(5)
    src = np.round(rng.normal(size=(400, 3)) * 64) / 8
    q = np.array([0.18, -0.32, 0.46, 0.0])
    q[3] = np.sqrt(1 - (q[:3] ** 2).sum())
    dst = np.round(ac.apply(np.concatenate([q, [1.0, 2.0, 3.0], [1.5]]), src) * 8) / 8
    ok0, S0, _, _ = oracle.align_sim3(src, dst, 127)
    for shift_a, shift_b in (([2.0 ** 22, 0, 0], [0, 2.0 ** 21, 0]), ([-2.0 ** 17, 2.0 ** 17, 2.0 ** 10], [2.0 ** 12, 0, -2.0 ** 17])):
        ok, S, _, _ = oracle.align_sim3(src + shift_a, dst + shift_b, 127)
        assert ok and ok0 and np.abs(ac.rotmat(S[:4]) - ac.rotmat(S0[:4])).max() < 1e-13 and abs(S[7] - S0[7]) < 1e-13 * S0[7]
        moved = S0[4:7] + shift_b - S0[7] * ac.rotmat(S0[:4]) @ shift_a
        assert np.abs(S[4:7] - moved).max() <= 1e-13 * max(np.linalg.norm(shift_a), np.linalg.norm(shift_b))
