"""Adversarial remap tables and images for the undistortion (gh_undistort_dev / _host): the table entries a smooth lens model
almost never produces (tests/test_undist_adversarial_oracle.py takes the census and pins the oracle,
tests/test_undist_adversarial_gpu.py holds the kernel to the oracle).  numpy only, seeded.

Tables are built from a source position (u, v) per output pixel by the reference's own float32 post-processing
(GSLAM/core/Undistorter.h:151-199, written out in tables_from_positions): a position outside [0, w_in) x [0, h_in) is
"bad" (remapX = remapFast = -1, indices and coefficients 0); otherwise remapX = float(u), remapFast = (int)u + w_in *
(int)v, and from the float32 fractions xx, yy and xxyy = xx * yy the indices (yyi * w_in + xxi, + 1, next row, + 1) and the
coefficients (1 - xx - yy + xxyy, xx - xxyy, yy - xxyy, xxyy).  Positions are float32-exact, so the (int) of the double
and of the float agree and the tables stay within what that post-processing produces.

CASES[name]() -> dict(tables, images: [(label, {1: H x W, 3: H x W x 3, 4: H x W x 4})])
REF_PAIRS[name] = (cam_in, cam_out): pinhole cameras with power-of-two focal lengths, through which the reference's own
prepareReMap reaches the same places exactly (u = x + dx, v = y + dy).
Builders are cached: the arrays are shared and must not be written to."""
import functools

import numpy as np

F32 = np.float32
W_IN, H_IN = 24, 16
BELOW_ONE = float(np.nextafter(F32(1), F32(0)))
FRACTIONS = (0.0, 2.0 ** -24, 0.5, BELOW_ONE)
MODES = ((1, False), (1, True), (3, False), (3, True), (4, True))  # (channels, fast); 4 channels bilinear is refused

CASES = {}


def _register(name):
    def deco(fn):
        CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def tables_from_positions(u, v, w_in, h_in, w_out, h_out):
    u, v = np.asarray(u, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    n = w_out * h_out
    assert len(u) == len(v) == n
    bad = (u < 0) | (v < 0) | (u >= w_in) | (v >= h_in)
    assert (bad | ((u.astype(F32) == u) & (v.astype(F32) == v))).all(), "positions must be float32-exact"
    X = np.where(bad, -1.0, u).astype(F32)
    Y = np.where(bad, -1.0, v).astype(F32)
    fast = np.where(bad, -1, np.trunc(np.where(bad, 0, u)).astype(np.int64) + w_in * np.trunc(np.where(bad, 0, v)).astype(np.int64)).astype(np.int32)
    xxi, yyi = X.astype(np.int32), Y.astype(np.int32)  # truncation; only used where not bad
    xx, yy = X - xxi.astype(F32), Y - yyi.astype(F32)
    xxyy = xx * yy
    assert xx.dtype == yy.dtype == xxyy.dtype == np.float32
    idx = np.stack([yyi * w_in + xxi, yyi * w_in + xxi + 1, (yyi + 1) * w_in + xxi, (yyi + 1) * w_in + xxi + 1], axis=1).astype(np.int32)
    one = F32(1)
    coef = np.stack([one - xx - yy + xxyy, xx - xxyy, yy - xxyy, xxyy], axis=1)
    assert coef.dtype == np.float32
    idx[bad], coef[bad] = 0, 0
    return dict(remapX=X, remapY=Y, remapFast=fast, remapIdx=idx, remapCoef=coef, w_in=w_in, h_in=h_in, w_out=w_out, h_out=h_out)


def images(w, h, seed, kind="random"):
    """{channels: image}; pixel 0 is non-zero in every channel."""
    rng = np.random.default_rng(seed)
    out = {}
    for ch in (1, 3, 4):
        shape = (h, w) if ch == 1 else (h, w, ch)
        if kind == "white":
            img = np.full(shape, 255, np.uint8)
        elif kind == "checker":
            yy, xx = np.mgrid[:h, :w]
            img = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
            img = img if ch == 1 else np.repeat(img[:, :, None], ch, axis=2).copy()
            if ch > 1:
                img[:, :, 1] = 255 - img[:, :, 1]
        else:
            img = rng.integers(0, 256, shape, dtype=np.uint8)
        img.reshape(-1)[:ch] = np.maximum(img.reshape(-1)[:ch], 1 + np.arange(ch, dtype=np.uint8) * 7)
        out[ch] = img
    return out


def _fill(rng, pos, n, w_in, h_in, step=0.25, outside=0.1):
    """pad the hand-placed positions with seeded ones on a grid of `step`, a share of them outside the image"""
    pos = list(pos)
    while len(pos) < n:
        u, v = rng.integers(0, int(w_in / step)) * step, rng.integers(0, int(h_in / step)) * step
        if rng.random() < outside:
            u, v = [(-step, v), (u, -1.0), (float(w_in), v), (u, h_in + 3.0)][rng.integers(0, 4)]
        pos.append((u, v))
    p = np.array(pos, np.float64)
    return p[:, 0], p[:, 1]


@_register("origin")
def origin():
    """Source pixel 0 and the first source column: remapX = 0.0 with remapFast = 0 and > 0, remapX = -0.0, remapX > 0 with
    remapFast = 0: where the five write rules part."""
    w_out, h_out = 12, 8
    rng = np.random.default_rng(301)
    pos = [(0.0, 0.0), (-0.0, 0.0), (0.0, 1.0), (0.0, 2.5), (0.0, 15.0), (-0.0, 3.0), (-0.0, 7.75), (0.5, 0.0), (0.75, 0.5),
           (1.0, 0.0), (0.25, 0.75), (2.0 ** -24, 0.0), (0.0, 2.0 ** -24), (-0.5, 3.0), (-2.0 ** -149, 0.0), (3.0, -2.0 ** -149)]
    u, v = _fill(rng, pos, w_out * h_out, W_IN, H_IN)
    return dict(tables=tables_from_positions(u, v, W_IN, H_IN, w_out, h_out), images=[("random", images(W_IN, H_IN, 311))])


@_register("last_row_col")
def last_row_col():
    """Positions in the last source row (the next-row indices lie past the image and clamp to the last pixel) and in the
    last source column (the + 1 indices step to the next row's first pixel, inside the image); (23, 15) does both and
    reaches n_in + w_in, the largest index the reference's tables hold."""
    w_out, h_out = 12, 8
    rng = np.random.default_rng(302)
    pos = [(x, 15.0) for x in (0.0, 1.0, 7.0, 22.0)] + [(x + 0.5, 15.25) for x in (0.0, 4.0, 11.0, 22.0)]
    pos += [(23.0, y) for y in (0.0, 1.0, 8.0, 14.0)] + [(23.5, y + 0.5) for y in (0.0, 3.0, 14.0)]
    pos += [(23.0, 15.0), (23.75, 15.75), (23.5, 15.0), (23.0, 15.5), (float(np.nextafter(F32(24), F32(0))), float(np.nextafter(F32(16), F32(0))))]
    u, v = _fill(rng, pos, w_out * h_out, W_IN, H_IN)
    return dict(tables=tables_from_positions(u, v, W_IN, H_IN, w_out, h_out), images=[("random", images(W_IN, H_IN, 312))])


@_register("fractions")
def fractions():
    """Every pair of the fractions 0, 2^-24, 0.5 and the float below 1 (at the origin, where float32 holds them), 0 and 0.5
    elsewhere, and seeded multiples of 2^-19; on an all-255 image, a 0 / 255 checkerboard and a random one."""
    w_out, h_out = 16, 12
    rng = np.random.default_rng(303)
    pos = [(fx, fy) for fx in FRACTIONS for fy in FRACTIONS]
    pos += [(x + fx, y + fy) for x, y in ((1.0, 1.0), (7.0, 3.0), (22.0, 14.0)) for fx in (0.0, 0.5) for fy in (0.0, 0.5)]
    pos += [(1.0, fy) for fy in FRACTIONS] + [(fx, 2.0) for fx in FRACTIONS]
    while len(pos) < w_out * h_out:
        pos.append((rng.integers(0, 15) + rng.integers(0, 2 ** 19) * 2.0 ** -19, rng.integers(0, 15) + rng.integers(0, 2 ** 19) * 2.0 ** -19))
    p = np.array(pos, np.float64)
    t = tables_from_positions(p[:, 0], p[:, 1], W_IN, H_IN, w_out, h_out)
    return dict(tables=t, images=[(k, images(W_IN, H_IN, 313, k)) for k in ("white", "checker", "random")])


@_register("all_bad")
def all_bad():
    """Every position lies outside the image: all modes give all zeros."""
    w_out, h_out = 9, 7
    pos = [(-1.0, -1.0), (24.0, 3.0), (3.0, 16.0), (-0.25, 5.0), (1e6, 1e6), (-2.0 ** -100, 2.0), (5.0, -2.0 ** -149), (-1e30, 4.0), (24.0, 16.0)]
    p = np.array([pos[i % len(pos)] for i in range(w_out * h_out)], np.float64)
    return dict(tables=tables_from_positions(p[:, 0], p[:, 1], W_IN, H_IN, w_out, h_out), images=[("random", images(W_IN, H_IN, 314))])


def _tiny(w_out, h_out, w_in, h_in, seed):
    rng = np.random.default_rng(seed)
    u, v = _fill(rng, [(0.0, 0.0), (w_in - 1.0, h_in - 1.0), (0.5, 0.5)][:min(3, w_out * h_out)], w_out * h_out, w_in, h_in, outside=0.15)
    order = rng.permutation(w_out * h_out) if w_out * h_out > 1 else np.array([0])
    return dict(tables=tables_from_positions(u[order], v[order], w_in, h_in, w_out, h_out), images=[("random", images(w_in, h_in, seed + 10))])


TINY = {"tiny_1x1": (1, 1, 2, 2), "tiny_17x15": (17, 15, 5, 3), "tiny_16x16": (16, 16, 2, 2), "tiny_257x1": (257, 1, 5, 3),
        "tiny_19x27": (19, 27, 2, 2)}
for _name, _dims in TINY.items():
    CASES[_name] = functools.lru_cache(maxsize=None)(functools.partial(_tiny, *_dims, 320 + len(_name) + _dims[0]))


def case(name):
    return CASES[name]()


# Pinhole pairs [w, h, fx, fy, cx, cy] with fx = fy = 16: u = x + (cx_in - cx_out), v = y + (cy_in - cy_out), exactly.
# The full 24 x 16 identity is not used: the 3-channel bilinear rule leaves its first column AND its last row out of the
# reference comparison, 39 of 384 pixels (10.2 %); the pairs below stay at or under 6.25 % in every mode.
REF_PAIRS = {
    "origin": ([24, 16, 16, 16, 8, 8], [24, 15, 16, 16, 8, 8]),             # u = x, v = y: pixel 0, first column, last column
    "last_row_col": ([24, 16, 16, 16, 8, 8], [23, 16, 16, 16, 7, 8]),       # u = x + 1, v = y: last row and last column
    "fractions": ([24, 16, 16, 16, 8, 8], [23, 15, 16, 16, 7.5, 7.5]),      # u = x + 0.5, v = y + 0.5
}


def ref_positions(name):
    cam_in, cam_out = REF_PAIRS[name]
    w_out, h_out = cam_out[0], cam_out[1]
    y, x = np.mgrid[:h_out, :w_out]
    return (x + (cam_in[4] - cam_out[4])).reshape(-1).astype(np.float64), (y + (cam_in[5] - cam_out[5])).reshape(-1).astype(np.float64)


def ref_tables(name):
    cam_in, cam_out = REF_PAIRS[name]
    u, v = ref_positions(name)
    return tables_from_positions(u, v, cam_in[0], cam_in[1], cam_out[0], cam_out[1])


@functools.lru_cache(maxsize=None)
def ref_images(name):
    cam_in = REF_PAIRS[name][0]
    return images(cam_in[0], cam_in[1], 330 + len(name))
