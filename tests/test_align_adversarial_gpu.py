"""gh_align_sim3 (align_sums_kernel / align_info_kernel, posegraph.hip) held to oracle_align_sim3 on the census of
tests/align_cases.py, and to the generating transform on its noise-free cases.

Bars.  GPU against oracle: 1e-11 in the three measures of align_cases.errors (rotation max |R - R*|, scale relative,
translation relative to max(1, |centroid of dst|)) -- the bar test_alignment_parity holds at the origin; `ok` equal; the
information matrix and ssq at that test's relative bars (1e-10 of max(1, largest entry) / max(1, ssq)).  The kernel and
the oracle compute the same sums about the same pivot and differ in the order of the fold only (per 256-block tree, then
block order, against one sequential loop), so what is left between them is summation-order rounding.  Collinear clouds
leave the rotation about the line free, and the two folds pick different members of a two-fold eigenspace: there the
image of the points is compared (1e-11 relative to max(1, |centroid of dst|)), and ssq.

GPU against the truth, noise-free cases: max(16 * e_c, 1e-11) per measure, e_c = the error of the float64 two-pass
centred Horn of align_cases.horn_centred against the same truth -- the bar of tests/test_align_adversarial_oracle.py,
whose docstring holds the reasoning and the measured values (worst e_c 7.5e-12, at offset 4e6 m / spread 1 m).  It needs
no mpmath.

Each case runs twice and must return the same bytes (fixed-order fold), and a third time with information_out = NULL
and ssq_out = NULL, where the transform must again be the same bytes."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac

pytestmark = pytest.mark.gpu


def _transform_only(ctx, src, dst, dof):
    from gslam_amd import hip
    out, ok = np.full(8, np.nan), C.c_int(-1)
    ctx.check(hip.lib.gh_align_sim3(ctx.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), len(src), int(dof),
                                    out.ctypes.data_as(C.c_void_p), None, None, C.byref(ok)))
    return bool(ok.value), out


@pytest.mark.parametrize("case", ac.CASES, ids=ac.NAMES)
def test_alignment_census(ctx, oracle, case):
    from gslam_amd import posegraph
    name, src, dst, dof, truth = case
    oko, So, io, sso = oracle.align_sim3(src, dst, dof)
    okg, Sg, ig, ssg = posegraph.align_sim3(ctx, src, dst, dof)
    ok2, S2, i2, ss2 = posegraph.align_sim3(ctx, src, dst, dof)
    ok3, S3 = _transform_only(ctx, src, dst, dof)
    assert okg == oko == (not ac.expect_refused(name))
    assert (ok2, S2.tobytes(), i2.tobytes(), ss2) == (okg, Sg.tobytes(), ig.tobytes(), ssg)
    assert ok3 == okg and S3.tobytes() == Sg.tobytes()
    if not okg:
        assert Sg.tolist() == So.tolist() == ac.IDENTITY.tolist() and not ig.any() and ssg == 0.0
        return
    assert np.abs(ig - io).max() <= 1e-10 * max(1.0, np.abs(io).max()) and abs(ssg - sso) <= 1e-10 * max(1.0, sso)
    if ac.rotation_is_free(name):
        e_g, e_o = ac.image_error(Sg, src, dst), ac.image_error(So, src, dst)
        print("%s: image error gpu %.1e oracle %.1e" % (name, e_g, e_o))
        assert e_g <= 1e-11 and abs(Sg[7] - So[7]) <= 1e-11 * So[7]
        return
    e = ac.errors(Sg, So, dst)
    print("%s: gpu - oracle rot %.1e scale %.1e trans %.1e" % ((name,) + e))
    assert max(e) <= 1e-11, e
    assert Sg[3] >= 0.0 and (dof & 64 or Sg[7] == 1.0)
    if truth is not None:
        e_c = ac.errors(ac.horn_centred(src, dst, bool(dof & 64)), truth, dst)
        e_t = ac.errors(Sg, truth, dst)
        print("%s: gpu - truth rot %.1e scale %.1e trans %.1e | e_c %.1e %.1e %.1e" % ((name,) + e_t + e_c))
        for k in range(3):
            assert e_t[k] <= max(16.0 * e_c[k], 1e-11), (k, e_t, e_c)
