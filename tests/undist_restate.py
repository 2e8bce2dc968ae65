"""Plain numpy restatement of the five write rules of the undistortion remap (undistort_kernel, oracle_undistort), after
GSLAM/core/Undistorter.h:206-348, on the tables of :120-203:

    fast, 1 channel      out = img[remapFast]                      where remapFast > 0          (:236)
    fast, 3 channels     out = img[remapFast]                      where remapFast >= 0         (:249; the reference reads
                                                                   index -1 elsewhere, undefined and not restated)
    fast, 4 channels     out = img[remapFast]                      where remapX > 0             (:260)
    bilinear, 1 channel  out = (uchar)(p0*c0 + p1*c1 + p2*c2 + p3*c3)   unless remapX < 0 (then 0)  (:308)
    bilinear, 3 channels the same per channel                      where remapX > 0             (:333)

The sum is float32, every product rounded, added left to right, stored truncating.  Table indices >= n_in (the reference's
step past the last source row) read pixel n_in - 1.  Pixels no rule writes are 0.  `defined` marks the pixels whose value
the reference itself defines (it writes them, from inside the image); fast = True: the written ones; bilinear: the
written ones that needed no clamp (1 channel: the zeros of remapX < 0 are written too).

fused=True evaluates the sum with fused multiply-adds (one rounding per step, emulated in float64) and wrong="..." flips
one write rule; the census of tests/test_undist_adversarial_oracle.py uses both to show what a class separates."""
import numpy as np

F32 = np.float32


def write_mask(tables, ch, fast, wrong=None):
    """bool per output pixel: the rule of (ch, fast) copies / interpolates a source value there."""
    x, f = np.asarray(tables["remapX"], F32), np.asarray(tables["remapFast"], np.int32)
    if fast:
        if ch == 1:
            return f >= 0 if wrong == "fast1_ge" else f > 0
        if ch == 3:
            return f > 0 if wrong == "fast3_gt" else f >= 0
        return x >= 0 if wrong == "fast4_ge" else x > 0
    if ch == 1:
        return x > 0 if wrong == "bil1_gt" else ~(x < 0)
    return ~(x < 0) if wrong == "bil3_ge" else x > 0


def _sum4(p, c, fused):
    """p, c: n x 4 float32 -> n float32, left to right."""
    if not fused:
        acc = p[:, 0] * c[:, 0]
        for k in (1, 2, 3):
            acc = acc + p[:, k] * c[:, k]
            assert acc.dtype == np.float32
        return acc
    p64, c64 = p.astype(np.float64), c.astype(np.float64)  # 8-bit x 24-bit products are exact in float64
    acc = (p64[:, 0] * c64[:, 0]).astype(F32)
    for k in (1, 2, 3):
        acc = (p64[:, k] * c64[:, k] + acc.astype(np.float64)).astype(F32)
    return acc


def undistort(img, tables, fast, fused=False, wrong=None):
    """img H_in x W_in [x C] uint8 -> (out H_out x W_out [x C] uint8, defined H_out x W_out bool)."""
    img = np.asarray(img, np.uint8)
    ch = 1 if img.ndim == 2 else img.shape[2]
    n_in, n_out = tables["w_in"] * tables["h_in"], tables["w_out"] * tables["h_out"]
    src = img.reshape(n_in, ch)
    out = np.zeros((n_out, ch), np.uint8)
    ok = write_mask(tables, ch, fast, wrong)
    if fast:
        out[ok] = src[np.asarray(tables["remapFast"], np.int64)[ok]]
        defined = ok.copy()
    else:
        idx = np.asarray(tables["remapIdx"], np.int64).reshape(n_out, 4)
        coef = np.asarray(tables["remapCoef"], F32).reshape(n_out, 4)
        clamped = (idx >= n_in).any(axis=1)
        idx = np.minimum(idx, n_in - 1)
        for j in range(ch):
            v = _sum4(src[:, j][idx[ok]].astype(F32), coef[ok], fused)
            assert ((v >= 0) & (v < 256)).all()  # inside the range where the reference's float -> uchar store is defined
            out[ok, j] = v.astype(np.int32).astype(np.uint8)  # truncation
        defined = (ok & ~clamped) | (~ok if ch == 1 else False)
    shape = (tables["h_out"], tables["w_out"])
    return out.reshape(shape if ch == 1 else shape + (ch,)), np.asarray(defined, bool).reshape(shape)
