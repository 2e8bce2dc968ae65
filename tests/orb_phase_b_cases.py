"""Frames, CPU census and the skip rule for the phase-B skip of orb_select (gslam_amd/csrc/orb.hip, select_weak_cells).

The rule: where the two-phase detector runs, the workgroup of a (level, frame) counts the level's STRONG cells -- cells that
hold a strict 3 x 3 maximum of the score map above ini_th -- and redoes the cells that phase A marked only if that count is
below the level's quota.  Everything here is CPU only and built on the oracle's own pyramid and score map (oracle/orb_oracle.c);
tests/test_orb_phase_b_skip_cpu.py proves the rule on these frames, tests/test_orb_phase_b_skip_gpu.py runs them.

Every frame is flat (BG) outside x < SAFE_X, y < SAFE_Y, so that no level has a weak candidate in its last tile column or
row: there a tile's pass 1 also reads what lies beyond the image, and whether such a tile counts as flat is not predictable
from the image alone.  An isolated pixel of BG + d scores exactly d (see tests/test_orb_two_phase_gpu.py).
"""
import ctypes as C
import functools

import numpy as np

from oracle_lib import _ptr

W, H = 640, 480
BG = 100
EDGE, CELL, CAP = 19, 32, 32
INI_TH, MIN_TH = 20, 7
SAFE_X, SAFE_Y = 19 + 14 * 32, 19 + 8 * 32  # level-0 cells 0 .. 13 x 0 .. 7: 7 x 4 tiles
N_BATCH = 14
K_BATCH = 150      # quotas [33, 27, 23, 19, 16, 13, 11, 8] (test_batch_holds_every_case asserts quota[0])
K_STREAM = 8000


def _cell_xy(cx, cy):
    return EDGE + CELL * cx, EDGE + CELL * cy


TILES = [(tx, ty) for ty in range(4) for tx in range(7)]  # level-0 tiles inside the safe region, in raster order


def _weak_dots(img, cx, cy, rng):
    """two dots of score 12 in cell (cx, cy)"""
    x, y = _cell_xy(cx, cy)
    img[y + 6 + int(rng.integers(0, 3)), x + 7 + int(rng.integers(0, 3))] = BG + 12
    img[y + 20 + int(rng.integers(0, 3)), x + 19 + int(rng.integers(0, 3))] = BG + 12


def _strong_dot(img, cx, cy, rng):
    """one corner of score 100 in cell (cx, cy): every strong corner of a frame ties with every other"""
    x, y = _cell_xy(cx, cy)
    img[y + 12 + int(rng.integers(0, 4)), x + 10 + int(rng.integers(0, 4))] = BG + 100


def boundary_frame(n_strong, seed, weak_first=False):
    """Exactly n_strong strong cells at level 0, each with ONE corner of score 100 (the cut falls inside a tie bin), in tiles whose
    other cells hold weak dots (score 12), so that no used tile is flat at ini_th.  Two special tiles carry one strong cell
    each beside a weak cell with more than 64 scored pixels (30 % of its pixels 12 above the others) and one with more than 32
    candidates (a 4-px lattice of score-12 dots).  weak_first: the pair tiles start in the second tile row and the first row holds
    the special tiles, so the weak cells come first in cell order."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), BG, np.uint8)
    tiles = list(TILES[7:] + TILES[:7]) if weak_first else list(TILES)
    specials = [tiles.pop(), tiles.pop()]
    left = n_strong - len(specials)
    assert 0 <= left <= 2 * len(tiles)
    for tx, ty in tiles:
        if left <= 0:
            break
        _strong_dot(img, 2 * tx, 2 * ty, rng)
        _weak_dots(img, 2 * tx + 1, 2 * ty, rng)
        _weak_dots(img, 2 * tx, 2 * ty + 1, rng)
        if left >= 2:
            _strong_dot(img, 2 * tx + 1, 2 * ty + 1, rng)
        else:
            _weak_dots(img, 2 * tx + 1, 2 * ty + 1, rng)
        left -= 2
    # more than 64 scored pixels
    tx, ty = specials[0]
    x, y = _cell_xy(2 * tx, 2 * ty)
    img[y + 1:y + 31, x + 1:x + 31] = np.where(rng.random((30, 30)) < 0.3, BG + 12, BG)
    _strong_dot(img, 2 * tx + 1, 2 * ty + 1, rng)
    # more than 32 candidates
    tx, ty = specials[1]
    x, y = _cell_xy(2 * tx, 2 * ty)
    img[y:y + 32:4, x:x + 32:4] = BG + 12
    _strong_dot(img, 2 * tx + 1, 2 * ty + 1, rng)
    return img


def weak_region(n_second, seed, w=W, h=H, x1=SAFE_X, y1=SAFE_Y):
    """The weak_tiles texture of tests/test_orb_two_phase_gpu.py over rows .. y1, columns .. x1: every score 12, one corner
    of score 100 per 64 x 64 tile, and a second one (32 px down and right) in the first n_second tiles -- three (or two) cells
    of four are marked, with more than 64 scored pixels and more than 32 candidates."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), BG, np.uint8)
    img[:y1, :x1] = np.where(rng.random((y1, x1)) < 0.3, BG + 12, BG)
    k = 0
    for y in range(EDGE + 10, y1 - 42, 64):
        for x in range(EDGE + 10, x1 - 42, 64):
            for d in (0, 32)[:2 if k < n_second else 1]:
                img[y + d - 4:y + d + 5, x + d - 4:x + d + 5] = BG
                img[y + d, x + d] = BG + 100
            k += 1
    return img


def strong_grid(img, cy0, cy1, cx1, seed):
    """one corner of score 100 in every cell of rows cy0 .. cy1 - 1, columns .. cx1 - 1 (flat background there)"""
    rng = np.random.default_rng(seed)
    x, y = _cell_xy(cx1, cy1)
    img[EDGE + CELL * cy0:y, :x] = BG
    for cy in range(cy0, cy1):
        for cx in range(cx1):
            _strong_dot(img, cx, cy, rng)
    return img


def blobs(step, amp, seed):
    """5 x 5 blobs of +amp every `step` px over the safe region: corners that survive the pyramid, so upper levels hold
    strong cells too."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), BG, np.uint8)
    for y in range(EDGE + 8, SAFE_Y - 8, step):
        for x in range(EDGE + 8, SAFE_X - 8, step):
            xx, yy = x + int(rng.integers(0, 3)), y + int(rng.integers(0, 3))
            img[yy:yy + 5, xx:xx + 5] = BG + amp
    return img


def weak_only(seed):
    """weak dots alone: every tile is flat at ini_th, nothing is strong on any level"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), BG, np.uint8)
    for tx, ty in TILES[::2]:
        _weak_dots(img, 2 * tx, 2 * ty, rng)
    return img


def trap_frame(seed, n_strong=20, n_flat=16):
    """The flat-tile trap at level 0: n_strong strong cells in pair tiles whose other cells are marked weak cells with
    candidates (first tile rows), then n_flat cells with weak dots in tiles that hold nothing else -- flat at ini_th, so
    orb_fast_cells finishes them single-phase with ordinary counts and scores <= ini_th.  strong < quota <= strong + n_flat:
    a count without the score test skips phase B, and the marked cells, which come first in cell order, lose their
    keypoints to the flat-tile cells."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), BG, np.uint8)
    tiles = list(TILES)
    for _ in range(n_strong // 2):
        tx, ty = tiles.pop(0)
        _strong_dot(img, 2 * tx, 2 * ty, rng)
        _strong_dot(img, 2 * tx + 1, 2 * ty + 1, rng)
        _weak_dots(img, 2 * tx + 1, 2 * ty, rng)
        _weak_dots(img, 2 * tx, 2 * ty + 1, rng)
    left = n_flat
    for tx, ty in tiles:
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            if left > 0:
                _weak_dots(img, 2 * tx + dx, 2 * ty + dy, rng)
                left -= 1
    return img


@functools.lru_cache(maxsize=None)
def batch_kinds(q0):
    """The boundary batch for quota[0] = q0: (kind, level-0 strong cells or None)."""
    return (("boundary", q0 - 1), ("boundary", q0), ("boundary", q0 + 1), ("weak_region", None), ("blobs", None),
            ("boundary_weak_first", q0 - 1), ("boundary_weak_first", q0), ("boundary_weak_first", q0 + 1), ("weak_only", None),
            ("blobs_small", None), ("boundary", q0 - 1), ("boundary", q0), ("boundary", q0 + 1), ("weak_region_short", None))


@functools.lru_cache(maxsize=None)
def batch_frames(q0):
    out = []
    for i, (kind, n) in enumerate(batch_kinds(q0)):
        out.append(boundary_frame(n, 300 + i) if kind == "boundary" else
                   boundary_frame(n, 300 + i, weak_first=True) if kind == "boundary_weak_first" else
                   weak_region(q0, 300 + i) if kind == "weak_region" else       # 28 tiles, two corners each: 56 strong cells
                   weak_region(0, 300 + i) if kind == "weak_region_short" else  # one each: 28 < q0
                   blobs(40, 60, 300 + i) if kind == "blobs" else
                   blobs(23, 45, 300 + i) if kind == "blobs_small" else weak_only(300 + i))
    fr = np.stack(out)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def trap_frames():
    fr = np.stack([trap_frame(500 + i) for i in range(N_BATCH)])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def stream_frames():
    """2 x 2560x1440 for K = 8000: level 0 has 79 x 44 = 3476 cells, two gathering rounds (cells 0 .. 2047 are rows 0 .. 25).
    Frame 0: weak texture with one strong corner per tile over cell rows 0 .. 9, a strong corner in every cell of rows 10 ..
    39 -- neither round's cells alone reach quota[0], both together do.  Frame 1: the weak texture alone: short of the quota,
    phase B redoes three cells of four."""
    w, h = 2560, 1440
    x1, y1 = _cell_xy(74, 40)
    f0 = strong_grid(weak_region(0, 700, w, h, x1, EDGE + 10 * CELL), 10, 40, 74, 702)
    f1 = weak_region(0, 701, w, h, x1, y1)
    fr = np.stack([f0, f1])
    fr.setflags(write=False)
    return fr


# ------------------------------------------------------------------------------------------------ census and rule
def compass(img, t):
    """Pass 1 of the detector at threshold t (tests/test_orb_two_phase_gpu.py)."""
    I = img.astype(np.int32)
    c = I[3:-3, 3:-3]
    u, d, l, r = I[:-6, 3:-3], I[6:, 3:-3], I[3:-3, :-6], I[3:-3, 6:]
    out = np.zeros(img.shape, bool)
    out[3:-3, 3:-3] = (((u > c + t) | (d > c + t)) & ((l > c + t) | (r > c + t))) | (((u < c - t) | (d < c - t)) & ((l < c - t) | (r < c - t)))
    return out


def _per_cell(a, ncx, ncy):
    """sum of a 2-d map (valid region only, origin at the first cell) over 32 x 32 cells -> [ncy, ncx]"""
    p = np.zeros((ncy * CELL, ncx * CELL), np.int64)
    p[:a.shape[0], :a.shape[1]] = a
    return p.reshape(ncy, CELL, ncx, CELL).sum(axis=(1, 3))


def score_map(oracle, lvl, min_th):
    """The oracle's score map of a level (0 outside the valid region and at or below min_th)."""
    return oracle.orb_score_map(lvl, min_th)


def level_census(oracle, lvl, ini_th=INI_TH, min_th=MIN_TH):
    """One pyramid level -> dict: S (the score map), ncx, ncy and [ncy, ncx] maps nz, cand, strong_cand, and `flat`: the cell's
    64 x 64 tile holds no compass survivor at ini_th in the window that pass 1 of orb_fast_cells tests (rows y0 - 1 .. y0 + 64,
    columns x0 - 3 .. x0 + 64), read inside the image.  None for a level without cells."""
    h, w = lvl.shape
    vw, vh = w - 2 * EDGE, h - 2 * EDGE
    if vw <= 0 or vh <= 0:
        return None
    S = score_map(oracle, lvl, min_th)
    Si = S.astype(np.int32)
    P = np.pad(Si, 1)
    nb = np.max([P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
    cand = (Si > 0) & (Si > nb)
    ncx, ncy = (vw + CELL - 1) // CELL, (vh + CELL - 1) // CELL
    v = (slice(EDGE, h - EDGE), slice(EDGE, w - EDGE))
    d = {"S": S, "ncx": ncx, "ncy": ncy, "nz": _per_cell(Si[v] > 0, ncx, ncy), "cand": _per_cell(cand[v], ncx, ncy),
         "strong_cand": _per_cell((cand & (Si > ini_th))[v], ncx, ncy)}
    surv = compass(lvl, ini_th)
    flat = np.zeros((ncy, ncx), bool)
    for by in range((ncy + 1) // 2):
        for bx in range((ncx + 1) // 2):
            x0, y0 = _cell_xy(2 * bx, 2 * by)
            flat[2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = not surv[y0 - 1:y0 + 65, x0 - 3:x0 + 65].any()
    d["flat"] = flat
    return d


def frame_census(oracle, img, nlevels=8, ini_th=INI_TH, min_th=MIN_TH):
    return [level_census(oracle, img if l == 0 else oracle.orb_pyramid_level(img, l, nlevels), ini_th, min_th) for l in range(nlevels)]


def strong_cells(c):
    """The kernel's count: a cell whose record holds 1 .. CAP entries and whose first entry scores above ini_th.  A cell keeps
    only its candidates above ini_th once it has one (oracle step 4), so this is: the cell holds a strong candidate."""
    return int((c["strong_cand"] > 0).sum())


def skips(c, quota):
    """The rule.  quota 0: orb_select returns before phase B."""
    return quota > 0 and strong_cells(c) >= quota


def predicted_weak_cells(c, quota, two_phase=True):
    """What one (level, frame) adds to the weak_cells debug counter: cells with candidates and no strong one that some kernel
    processes at min_th -- all of them where phase B runs (or the call is single-phase); only those of flat tiles, which
    orb_fast_cells finishes itself, where phase B is skipped.  quota 0: no fast_cells launch for the level at all."""
    if c is None or quota <= 0:
        return 0
    weak = (c["cand"] > 0) & (c["strong_cand"] == 0)
    if two_phase and skips(c, quota):
        weak = weak & c["flat"]
    return int(weak.sum())


def last_tiles(c):
    """[ncy, ncx] mask of the cells in the last tile column or row of the level"""
    m = np.zeros((c["ncy"], c["ncx"]), bool)
    m[2 * ((c["ncy"] - 1) // 2):, :] = True
    m[:, 2 * ((c["ncx"] - 1) // 2):] = True
    return m


def predictable(c, quota):
    """The prediction above does not depend on what lies beyond the image: in a skipped (level, frame), no weak cell with
    candidates sits in a last-column / last-row tile that looks flat from inside the image."""
    if c is None or quota <= 0 or not skips(c, quota):
        return True
    weak = (c["cand"] > 0) & (c["strong_cand"] == 0)
    return not (weak & c["flat"] & last_tiles(c)).any()


def select_level(oracle, S, ini_th, quota):
    """oracle_orb_select_level on a score map -> [n, 3] int32 (x, y, s) in output order"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    h, w = S.shape
    xs, ys, ss = (np.zeros(max(quota, 1), np.int32) for _ in range(3))
    oracle.lib.oracle_orb_select_level.restype = C.c_int
    n = oracle.lib.oracle_orb_select_level(_ptr(S), int(w), int(h), int(ini_th), int(quota), _ptr(xs), _ptr(ys), _ptr(ss))
    return np.stack([xs[:n], ys[:n], ss[:n]], axis=1)


def without_weak_cells(c, keep=None):
    """The level's score map with every score zeroed in the cells that hold no strong candidate (except where keep[cy, cx])."""
    S = c["S"].copy()
    h, w = S.shape
    for cy, cx in np.argwhere(c["strong_cand"] == 0):
        if keep is not None and keep[cy, cx]:
            continue
        x, y = _cell_xy(cx, cy)
        S[y:min(y + CELL, h - EDGE), x:min(x + CELL, w - EDGE)] = 0
    return S
