"""GPU parity of the two-phase FAST detector on the per-level path of gh_orb_extract_dev (gslam_amd/csrc/orb.hip).

Where ini_th > min_th, orb_fast_cells scores a level at ini_th only (phase A) and marks every cell that holds no candidate above
ini_th; orb_select redoes the marked cells at min_th, one wave per cell, before it reads the records (phase B).  The frames
here are built so that every way a cell can end up marked certainly occurs -- checked on the CPU with the oracle's own score
map before anything runs on the GPU -- and every comparison is bit-exact on all 28 + 32 bytes of every record, the counts
and the zero tail against oracle.orb_extract_batch, as in tests/test_orb_per_level_gpu.py.

A tile in which nothing passes the compass test at ini_th is finished single-phase inside orb_fast_cells (the flat-tile
shortcut), so every cell that is meant for phase B shares its tile with a strong corner or an edge, and the CPU checks assert
that the tile's window holds a compass survivor at ini_th.

An isolated pixel of value bg + d on a flat background scores exactly d and nothing around it scores (its ring differs from
it by d everywhere; any other pixel sees it in at most two adjacent ring positions), so dots place scores at will.
"""
import functools

import numpy as np
import pytest

from orb_images import CLASSES, noise
from test_orb_per_level_gpu import _gpu, _oracle, _prefix, _same, overlap, per_level

pytestmark = pytest.mark.gpu

W, H = 640, 480
BG = 100
EDGE, CELL = 19, 32
N_PER_LEVEL, N_OVERLAP, N_SMALL = 14, 55, 13
# (ini_th, min_th) -> two-phase?
THRESHOLDS = [((20, 7), True), ((254, 1), True), ((7, 7), False), ((9, 8), True), ((5, 9), False), ((254, 254), False)]


def _cell_xy(cx, cy):
    return EDGE + CELL * cx, EDGE + CELL * cy


def constructed(seed):
    """A 640x480 frame (level 0: 19 x 14 cells, the last column and row 26 px wide / high) with, at level 0 and (ini_th, min_th)
    = (20, 7), the cell classes named in test_constructed_frame_holds_every_class.  `seed` moves the dots inside their cells."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), BG, np.uint8)
    j = lambda: int(rng.integers(0, 4))

    def dot(x, y, amp):
        img[y, x] = BG + amp

    # weak cell (2, 2): three dots of score 12; its neighbour (3, 2) holds a strong corner
    x, y = _cell_xy(2, 2)
    for k in range(3):
        dot(x + 5 + 9 * k + j(), y + 6 + 8 * k + j(), 12)
    x, y = _cell_xy(3, 2)
    dot(x + 10 + j(), y + 12 + j(), 100)
    # cell (5, 2): its only pixel above ini_th sits in its last column and loses to its right neighbour in cell (6, 2)
    x, y = _cell_xy(6, 2)
    yy = y + 10 + j()
    dot(x - 1, yy, 30)
    dot(x, yy, 60)
    dot(x - 20 + j(), y + 24, 12)
    # the same downwards: last row of cell (8, 2) against the first row of cell (8, 3)
    x, y = _cell_xy(8, 3)
    xx = x + 9 + j()
    dot(xx, y - 1, 30)
    dot(xx, y, 60)
    dot(x + 25, y - 20 + j(), 12)
    # equal scores across the border: with strict NMS neither is a candidate -- cells (11, 2) | (12, 2) and (14, 2) / (14, 3)
    x, y = _cell_xy(12, 2)
    yy = y + 15 + j()
    dot(x - 1, yy, 40)
    dot(x, yy, 40)
    dot(x - 16 + j(), y + 4, 12)
    x, y = _cell_xy(14, 3)
    xx = x + 14 + j()
    dot(xx, y - 1, 40)
    dot(xx, y, 40)
    dot(x + 3, y - 12 + j(), 12)
    # weak partial cells: the last cell column (18, 5), the last cell row (9, 13) and the corner (18, 13) -- ncx = 19 is odd,
    # so column 18 is the only cell column of its tile
    for cx, cy in ((18, 5), (9, 13), (18, 13)):
        x, y = _cell_xy(cx, cy)
        dot(x + 8 + j(), y + 9 + j(), 12)
        dot(x + 20 + j(), y + 18 + j(), 9)
        x, y = _cell_xy(cx, cy - 1)  # a strong corner in the cell above, in the same tile: the tile is not flat at ini_th
        dot(x + 10 + j(), y + 12 + j(), 100)
    # low-contrast noise over cells (3 .. 4, 6 .. 7), 30 % of the pixels 12 above the others: weak cells with more than 64
    # scored pixels, every score 12 (uniform noise of +- 9 or +- 10 scores only ~30 pixels of a cell); a strong corner in the
    # other cell column of each of the two tiles, (2, 6) and (5, 7), so that neither tile is flat at ini_th
    x, y = _cell_xy(3, 6)
    img[y:y + 64, x:x + 64] = np.where(rng.random((64, 64)) < 0.3, BG + 12, BG)
    for cx, cy in ((2, 6), (5, 7)):
        x, y = _cell_xy(cx, cy)
        dot(x + 10 + j(), y + 12 + j(), 100)
    # a 4-px lattice of score-12 dots over cell (8, 6): a weak cell with 64 equal candidates (cap 32); a strong corner in (9, 7)
    x, y = _cell_xy(8, 6)
    for dy in range(0, 32, 4):
        for dx in range(0, 32, 4):
            dot(x + dx, y + dy, 12)
    x, y = _cell_xy(9, 7)
    dot(x + 10 + j(), y + 12 + j(), 100)
    # 5 x 5 blobs of +18 over the lower left: they survive the pyramid as low-contrast corners, which puts weak cells into the
    # last cell row of levels 5 and 7, whose ncy (5 and 3) is odd
    for yy in range(330, 455, 17):
        for xx in range(25, 290, 17):
            img[yy:yy + 5, xx:xx + 5] = BG + 18
    # a diagonal band of +30 through the tile of cells (14 .. 15, 10 .. 11), its ends in other tiles, and two dots of score 12:
    # pixels along the edges pass the compass test at ini_th, none of the tile scores above it (an edge is no corner)
    x, y = _cell_xy(14, 10)
    yy, xx = np.mgrid[y - 45:y + 109, 0:W]
    band = img[y - 45:y + 109]
    band[(xx + yy >= x + y + 54) & (xx + yy < x + y + 74)] = BG + 30
    dot(x + 13 + j(), y + 6, 12)
    dot(x + 33 + j(), y + 56, 12)
    # a textured tile (cells 12 .. 13, 6 .. 7) beside a completely flat one (cells 14 .. 15, 6 .. 7)
    x, y = _cell_xy(12, 6)
    img[y:y + 64, x:x + 64] = noise(64, 64, seed + 2)
    return img


def compass(img, t):
    """Pass 1 of the detector at threshold t: two adjacent compass pixels (distance 3) both brighter than c + t or both darker
    than c - t.  -> bool map (False within 3 px of the image border)."""
    I = img.astype(np.int32)
    c = I[3:-3, 3:-3]
    u, d, l, r = I[:-6, 3:-3], I[6:, 3:-3], I[3:-3, :-6], I[3:-3, 6:]
    out = np.zeros(img.shape, bool)
    out[3:-3, 3:-3] = (((u > c + t) | (d > c + t)) & ((l > c + t) | (r > c + t))) | (((u < c - t) | (d < c - t)) & ((l < c - t) | (r < c - t)))
    return out


def census(oracle, img, ini_th, min_th, nlevels=8):
    """Per level: dict of [ncy, ncx] arrays -- nz (pixels with S > 0), strong_px (S > ini_th), cand (strict 3 x 3 maxima),
    strong_cand (those above ini_th) -- from the oracle's pyramid and score map."""
    out = []
    for l in range(nlevels):
        lvl = img if l == 0 else oracle.orb_pyramid_level(img, l, nlevels)
        h, w = lvl.shape
        vw, vh = w - 2 * EDGE, h - 2 * EDGE
        if vw <= 0 or vh <= 0:
            out.append(None)
            continue
        S = oracle.orb_score_map(lvl, min_th).astype(np.int32)
        valid = np.zeros_like(S, bool)
        valid[EDGE:h - EDGE, EDGE:w - EDGE] = True
        S = np.where(valid & (S > min_th), S, 0)
        P = np.pad(S, 1)
        nb = np.max([P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
        cand = (S > 0) & (S > nb)
        ncx, ncy = (vw + CELL - 1) // CELL, (vh + CELL - 1) // CELL
        d = {k: np.zeros((ncy, ncx), np.int32) for k in ("nz", "strong_px", "cand", "strong_cand")}
        for cy in range(ncy):
            for cx in range(ncx):
                x, y = _cell_xy(cx, cy)
                s, c = S[y:min(y + CELL, h - EDGE), x:min(x + CELL, w - EDGE)], cand[y:min(y + CELL, h - EDGE), x:min(x + CELL, w - EDGE)]
                d["nz"][cy, cx] = (s > 0).sum()
                d["strong_px"][cy, cx] = (s > ini_th).sum()
                d["cand"][cy, cx] = c.sum()
                d["strong_cand"][cy, cx] = (c & (s > ini_th)).sum()
        out.append(d)
    return out


def weak_tiles(w, h, seed):
    """30 % of the pixels 12 above the others (every score is 12) and one corner of score 100 in every 64 x 64 tile of level 0: no
    tile is flat at ini_th, and three cells of four are marked with more than 64 scored pixels and more than 32 candidates."""
    img = np.where(np.random.default_rng(seed).random((h, w)) < 0.3, BG + 12, BG).astype(np.uint8)
    for y in range(EDGE + 10, h - EDGE, 64):
        for x in range(EDGE + 10, w - EDGE, 64):
            img[y - 4:y + 5, x - 4:x + 5] = BG
            img[y, x] = BG + 100
    return img


NAMES = ["low_contrast", "few_corners", "step_edges", "mixed"]


def _frame_kinds(n):
    """Frame i of a batch: every third one built here (constructed / weak_tiles in turn), the others cycle through the four
    existing classes."""
    return [("constructed" if i % 6 == 0 else "weak_tiles") if i % 3 == 0 else NAMES[(i - i // 3 - 1) % 4] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _frames(n):
    """n frames: constructed and weak_tiles frames (every third) between the existing classes low_contrast, few_corners,
    step_edges, mixed (test_frame_mix_holds_every_class)."""
    out = []
    for i, kind in enumerate(_frame_kinds(n)):
        out.append(constructed(100 + i) if kind == "constructed" else weak_tiles(W, H, 100 + i) if kind == "weak_tiles"
                   else CLASSES[kind](W, H, 50 + i))
    fr = np.stack(out)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _expected(oracle, n, K, ini_th, min_th):
    return _oracle(oracle, _frames(n), K=K, ini_th=ini_th, min_th=min_th)


def test_constructed_frame_holds_every_class(oracle):
    """CPU only (the oracle's score map): the constructed frame really holds, at level 0 and (20, 7), each class of cell the
    two-phase detector must get right, and weak cells in the last cell row of an upper level with odd ncy."""
    img = constructed(100)
    c = census(oracle, img, 20, 7)[0]
    survivors = compass(img, 20)

    def weak(cx, cy):
        """Cell (cx, cy) has candidates and none above ini_th, and the 66 x 66 window of its tile holds a pixel that passes the
        compass test at ini_th: the tile is not finished single-phase by the flat-tile shortcut, the cell reaches phase B."""
        x, y = _cell_xy(cx - cx % 2, cy - cy % 2)
        return c["cand"][cy, cx] > 0 and c["strong_cand"][cy, cx] == 0 and survivors[y - 1:y + 65, x - 1:x + 65].any()
    assert c["nz"].shape == (14, 19)
    # all candidates in (min_th, ini_th], next to a cell with a strong corner
    assert weak(2, 2) and c["strong_px"][2, 2] == 0 and c["strong_cand"][2, 3] == 1
    # a strong pixel on the border that loses to a larger neighbour across it: weak although it holds a strong pixel
    assert weak(5, 2) and c["strong_px"][2, 5] == 1 and c["strong_cand"][2, 6] == 1
    assert weak(8, 2) and c["strong_px"][2, 8] == 1 and c["strong_cand"][3, 8] == 1
    # equal scores across the border: neither is a candidate, both cells are without a strong corner
    assert weak(11, 2) and c["strong_px"][2, 11] == 1 and c["strong_px"][2, 12] == 1 and c["strong_cand"][2, 12] == 0
    assert weak(14, 2) and c["strong_px"][2, 14] == 1 and c["strong_px"][3, 14] == 1 and c["strong_cand"][3, 14] == 0
    # weak partial cells in the last cell column / row (26 px) and the last tile of the odd ncx = 19
    assert weak(18, 5) and weak(9, 13) and weak(18, 13)
    # a completely flat tile beside a textured one
    assert c["nz"][6:8, 14:16].sum() == 0 and c["strong_cand"][6:8, 12:14].min() > 0
    # a tile with compass survivors at ini_th and no score above it, weak candidates inside
    assert c["strong_px"][10:12, 14:16].sum() == 0 and weak(14, 10) and weak(15, 11)
    # a weak cell with more than 64 scored pixels (phase B's list branch), all between 8 and 20
    assert weak(3, 6) and c["nz"][6, 3] > 64 and c["strong_px"][6, 3] == 0
    assert weak(4, 7) and c["nz"][7, 4] > 64 and c["strong_px"][7, 4] == 0
    # a weak cell with more than 32 candidates (cap)
    assert weak(8, 6) and c["cand"][6, 8] > 32
    # weak cells in the last cell row of a level with odd ncy (the blobs)
    upper = [d for d in census(oracle, img, 20, 7)[1:] if d is not None and d["nz"].shape[0] % 2 == 1]
    assert any(((d["cand"][-1] > 0) & (d["strong_cand"][-1] == 0)).any() for d in upper)


def test_frame_mix_holds_every_class(oracle):
    """CPU only: both batches hold all four existing classes beside the frames built here, and a weak_tiles frame sends cells
    with more than 64 scored pixels and with more than 32 candidates to phase B (no tile of it is flat at ini_th)."""
    for n in (N_PER_LEVEL, N_OVERLAP):
        assert set(_frame_kinds(n)) == set(NAMES) | {"constructed", "weak_tiles"}, _frame_kinds(n)
    i = _frame_kinds(N_PER_LEVEL).index("weak_tiles")
    img = np.array(_frames(N_PER_LEVEL)[i])
    c, survivors = census(oracle, img, 20, 7)[0], compass(img, 20)
    marked = (c["strong_cand"] == 0)
    for cy, cx in np.argwhere(marked):
        x, y = _cell_xy(cx - cx % 2, cy - cy % 2)
        assert survivors[y - 1:y + 65, x - 1:x + 65].any(), (cx, cy)
    assert (marked & (c["nz"] > 64)).sum() > 20 and (marked & (c["cand"] > 32)).sum() > 20  # (of 266 cells, ~196 marked)


@pytest.mark.parametrize("th,two", THRESHOLDS, ids=["ini%d-min%d" % t for t, _ in THRESHOLDS])
def test_thresholds_per_level(ctx, oracle, th, two):
    """14 x 640x480 (per-level, one select at the end) at every threshold pair: (20, 7), (254, 1) -- nearly every cell weak --
    and (9, 8) run two-phase; (7, 7) and (254, 254) single-phase; (5, 9) (ini_th < min_th) is refused at plan creation."""
    ini_th, min_th = th
    assert two == (ini_th > min_th)
    assert per_level(N_PER_LEVEL, W, H) and not overlap(N_PER_LEVEL, W, H)
    if ini_th < min_th:  # gh_orb_plan_create refuses such a pair, so the kernels' ini_th <= min_th guard only ever sees equality
        from gslam_amd.hip import GslamHipError
        with pytest.raises(GslamHipError, match="ini_th_fast >= prm.min_th_fast"):
            _gpu(ctx, np.array(_frames(N_PER_LEVEL)), ini_th=ini_th, min_th=min_th)
        return
    got, _ = _gpu(ctx, np.array(_frames(N_PER_LEVEL)), ini_th=ini_th, min_th=min_th)
    _same(got, _expected(oracle, N_PER_LEVEL, 1000, ini_th, min_th), f"{N_PER_LEVEL} x {W}x{H} ini_th={ini_th} min_th={min_th}")


@pytest.mark.parametrize("th", [(20, 7), (254, 1)], ids=["ini20-min7", "ini254-min1"])
def test_overlap_schedule(ctx, oracle, th):
    """55 x 640x480: select(l), and with it phase B of level l, runs on the side stream beside fast_cells(l + 1)."""
    ini_th, min_th = th
    assert overlap(N_OVERLAP, W, H)
    got, _ = _gpu(ctx, np.array(_frames(N_OVERLAP)), ini_th=ini_th, min_th=min_th)
    _same(got, _expected(oracle, N_OVERLAP, 1000, ini_th, min_th), f"{N_OVERLAP} x {W}x{H} ini_th={ini_th} min_th={min_th}")


def test_small_twin(ctx, oracle):
    """The first 13 frames of the batch through the small path (single-phase) give the records of the 14-frame per-level call."""
    assert not per_level(N_SMALL, W, H)
    big, _ = _gpu(ctx, np.array(_frames(N_PER_LEVEL)))
    _same(big, _expected(oracle, N_PER_LEVEL, 1000, 20, 7), f"{N_PER_LEVEL} x {W}x{H}")
    small, _ = _gpu(ctx, np.array(_frames(N_PER_LEVEL)[:N_SMALL]))
    _same(small, _prefix(big, N_SMALL), f"the {N_SMALL}-frame small twin")


def test_streamed_select(ctx, oracle):
    """2560x1440: level 0 has 3476 cells, more than the cached select holds, so the streaming select_kernel<false> runs and
    gathers its marked cells in two rounds.  One frame per call is a small call (3.7 Mpixel: single-phase); the per-level call
    that runs phase B in the streaming select is the same frame twice over, and both must give the oracle's records."""
    w, h = 2560, 1440
    assert not per_level(1, w, h) and per_level(2, w, h)
    f = CLASSES["low_contrast"](w, h, 9)
    f[:, w // 2:] = CLASSES["few_corners"](w - w // 2, h, 10)
    f[h // 2:, :w // 4] = noise(w // 4, h - h // 2, 11)
    f[:h // 2, w // 4:w // 2] = weak_tiles(w // 2 - w // 4, h // 2, 12)  # (marked cells that take phase B's list branch and cap)
    frames = np.stack([f, f[::-1].copy()])
    exp = _oracle(oracle, frames, K=8000)
    one, _ = _gpu(ctx, frames[:1], K=8000)
    _same(one, _prefix(exp, 1), f"1 x {w}x{h}")
    two, _ = _gpu(ctx, frames, K=8000)
    _same(two, exp, f"2 x {w}x{h}")


def test_counters(ctx, oracle):
    """The debug counters on the per-level path: every cell counted once, weak cells counted by phase B, and no strong corner
    ever silences a weaker one in phase A, which never sees one; the small twin (single-phase) does count them."""
    frames = np.array(_frames(N_PER_LEVEL))
    got, d = _gpu(ctx, frames, counters=True)
    _same(got, _expected(oracle, N_PER_LEVEL, 1000, 20, 7), "counters on")
    ws, hs = oracle.orb_level_dims(W, H, 8)
    cells = sum(((lw - 38 + 31) // 32) * ((lh - 38 + 31) // 32) for lw, lh in zip(ws.tolist(), hs.tolist()))
    assert d["cells"] == N_PER_LEVEL * cells, d
    assert d["weak_cells"] > 0 and d["strong_silenced"] == 0, d
    assert d["dense_cells"] > 0 and d["cap_cells"] > 0 and d["rank_dropped"] > 0 and d["overflow_cells"] > 0, d
    twin, ds = _gpu(ctx, frames[:N_SMALL], counters=True)
    _same(twin, _prefix(got, N_SMALL), "the small twin, counters on")
    assert ds["strong_silenced"] > 0 and ds["weak_cells"] > 0, ds
