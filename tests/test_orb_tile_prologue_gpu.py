"""GPU parity of the tile prologue of orb_fast_cells (gslam_amd/csrc/orb.hip: fast_cells_tile, TileHead, TileColRec).

A tile requests both of its 16-byte items per thread at once from the leading kernel arguments, then the advice word and the
packed record of its tile column and row together, then the operands of the fused MFMA resize.  None of it may change a byte:
every case runs on the per-level schedule (the first batch above 4 << 20 pixels) and compares counts, all 28 keypoint bytes,
the descriptors and the zero tail with oracle.orb_extract_batch.  The shapes are chosen by TILE GRID (64 x 64 tiles over the
region inside the 19-px border), each checked against the oracle's level geometry before it is relied on:
  96 x 96     one tile at level 0: every clamp of both items is active, the second item's rows run past the image
  160 x 192   2 x 3 tiles: exactly one interior tile takes the record-driven MFMA resize, the others the VALU path; the
              upper levels shrink to one tile
  64 k + 38 + {1, 15} wide: the last 16-byte window of a row is left to the pitch - 16 clamp, with row padding, read in place
              and staged (a base pointer that is not 16-byte aligned), the last frame of the batch included
A wrong record that silently fell back to the VALU resize would cost speed only, so the resize-pass census of two shapes is
held to the rule "MFMA passes on interior tiles, VALU passes on edge tiles", computed here from the plan's geometry.
"""
import functools

import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_images import CLASSES
from orb_phase_b_cases import INI_TH, K_BATCH, N_BATCH
from orb_threshold_hint_cases import textured_frames
from test_orb_per_level_gpu import _extract, _grid, _oracle, _plan, _same, first_per_level, overlap, per_level
from test_orb_phase_b_skip_gpu import _batch, _expected

pytestmark = pytest.mark.gpu

K = 1000
DISTINCT = ("noise", "mixed", "step_edges", "dots5", "binary_noise")  # cycled to the batch: the oracle runs five frames per shape


def _tiles(grid):
    return [((ncx + 1) // 2, (ncy + 1) // 2) for ncx, ncy in grid]


@functools.lru_cache(maxsize=None)
def _case(oracle, w, h, nlevels=8):
    """(the distinct frames, the batch cycled from them, the oracle's records for the batch)"""
    B = first_per_level(w, h)
    assert per_level(B, w, h) and not per_level(B - 1, w, h) and not overlap(B, w, h)
    five = np.stack([CLASSES[n](w, h, 77 + 13 * i + w) for i, n in enumerate(DISTINCT)])
    exp5 = _oracle(oracle, five, K=K, nlevels=nlevels)
    idx = np.arange(B) % len(DISTINCT)
    return five, five[idx], tuple(a[idx] for a in exp5)


def _pyramid_matches(ex, oracle, frames, what, nlevels=8):
    B = len(frames)
    for f in (0, B - 1):
        for l in range(1, nlevels):
            assert np.array_equal(ex.debug_level(f, l), oracle.orb_pyramid_level(frames[f], l)), f"{what}: pyramid level {l} of frame {f}"


def _extract_offset(ex, frames, stride, offset):
    """_extract with level 0 at `offset` bytes into its allocation and rows `stride` bytes apart; the bytes outside the images
    are noise"""
    import torch
    B, h, w = frames.shape
    flat = np.random.default_rng(stride + offset).integers(0, 256, offset + B * h * stride, dtype=np.uint8)
    flat[offset:].reshape(B, h, stride)[:, :, :w] = frames
    dev = torch.from_numpy(flat).cuda()
    view = dev[offset:].view(B, h, stride)
    assert view.data_ptr() % 16 == offset % 16
    kps, desc, counts = ex.extract(view)
    torch.cuda.synchronize()
    return kps.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()


# ---------------------------------------------------------------- the resize-pass census, from the plan's geometry
def _axis(n_src, n_dst):
    """source index per output column / row of a level (build_axis_table)"""
    out = []
    for x in range(n_dst):
        P = max(0, ((2 * x + 1) * n_src * 2048) // (2 * n_dst) - 1024)
        out.append(min(P >> 11, n_src - 1))
    return out


def expected_resize_passes(dims, quotas, B):
    """kDbgResizePasses of one per-level call on B frames: for every level with a FAST launch and a successor, an interior tile
    (not in the first / last tile row nor the last tile column) that owns at most 8 output groups counts one pass per wave with
    rows and per pair of column-block pairs (resize_tile_mfma); every other tile one per wave with items and per block of 8
    groups (the VALU loop of fast_cells_tile).  dims: (w, h) per level."""
    total = 0
    for l in range(len(dims) - 1):
        (w, h), (wd, hd) = dims[l], dims[l + 1]
        ncx, ncy = (max(0, w - 38) + 31) // 32, (max(0, h - 38) + 31) // 32
        if ncx == 0 or ncy == 0 or quotas[l] == 0:
            continue
        nbx, nby = (ncx + 1) // 2, (ncy + 1) // 2
        sx, sy, ngroups = _axis(w, wd), _axis(h, hd), (wd + 7) // 8
        # the 32-column K window of every group holds both taps of its 16 columns (build_mfma_tables), else no tile takes the MFMA path
        mfma = all(0 <= sx[x] - (sx[8 * g] & ~7) and min(sx[x] + 1, w - 1) - (sx[8 * g] & ~7) <= 31
                   for g in range(ngroups) for x in range(8 * g, min(8 * g + 16, wd)))
        gx, g = [], 0
        for bx in range(nbx + 1):  # build_own_tables
            if bx == nbx:
                g = ngroups
            else:
                while bx > 0 and g < ngroups and sx[8 * g] < 64 * bx:
                    g += 1
            gx.append(g)
        gy, y = [], 0
        for by in range(nby + 1):
            if by == nby:
                y = hd
            else:
                while by > 0 and y < hd and sy[y] < 64 * by + 15:
                    y += 1
            gy.append(y)
        for by in range(nby):
            for bx in range(nbx):
                ng, rows = gx[bx + 1] - gx[bx], gy[by + 1] - gy[by]
                if mfma and 0 < by < nby - 1 and bx < nbx - 1 and ng <= 8:
                    total += min(4, (rows + 15) // 16) * (((ng + 1) // 2 + 1) // 2)
                else:
                    total += ((ng + 7) // 8) * ((((rows + 3) // 4) + 7) // 8)
    return total * B


@pytest.mark.parametrize("w,h", [(160, 192), (167, 120)])
def test_resize_census_follows_the_tile_grid(ctx, oracle, w, h):
    """counters on (hints are off then): the records, the pyramid and the number of passes through either resize body"""
    five, frames, exp = _case(oracle, w, h)
    ex = _plan(ctx, w, h, len(frames), K)
    try:
        dims = [ex.level(l)[:2] for l in range(8)]
        quotas = [ex.level(l)[2] for l in range(8)]
        ws, hs = oracle.orb_level_dims(w, h, 8)
        assert dims == list(zip(ws.tolist(), hs.tolist()))
        got, d = _extract(ex, frames, pad=(-w) % 16, counters=True)
        _pyramid_matches(ex, oracle, frames, f"{w}x{h}")
    finally:
        ex.close()
    _same(got, exp, f"{len(frames)} x {w}x{h}, counters on")
    want = expected_resize_passes(dims, quotas, len(frames))
    print("resize passes", d["resize_passes"], "expected", want)
    assert d["resize_passes"] == want, (d, want)


# ---------------------------------------------------------------- tile grids
def test_single_tile_at_level_0(ctx, oracle):
    w = h = 96
    assert _tiles(_grid(oracle, w, h))[0] == (1, 1)
    five, frames, exp = _case(oracle, w, h)
    ex = _plan(ctx, w, h, len(frames), K)
    try:
        got, _ = _extract(ex, frames)
        _pyramid_matches(ex, oracle, frames, "96x96")
    finally:
        ex.close()
    _same(got, exp, f"{len(frames)} x 96x96")


@pytest.mark.parametrize("nlevels", [1, 8])
def test_exactly_one_interior_tile(ctx, oracle, nlevels):
    """160 x 192: tile (0, 1) of level 0 is the only interior tile of the pyramid.  One level: no successor, no record is read."""
    w, h = 160, 192
    tiles = _tiles(_grid(oracle, w, h))
    assert tiles[0] == (2, 3) and all(nby <= 2 or nbx == 1 for nbx, nby in tiles[1:]) and tiles[-1] == (1, 1), tiles
    five, frames, exp = _case(oracle, w, h, nlevels)
    ex = _plan(ctx, w, h, len(frames), K, nlevels=nlevels)
    try:
        got, _ = _extract(ex, frames, pad=(-w) % 16)
        _pyramid_matches(ex, oracle, frames, f"160x192, {nlevels} levels", nlevels)
    finally:
        ex.close()
    _same(got, exp, f"{len(frames)} x 160x192, {nlevels} levels")


@pytest.fixture(scope="module", params=[167, 181], ids=["w167", "w181"])
def clamp_plan(request, ctx, oracle):
    """64 * 2 + 38 + {1, 15}: the valid region ends 1 / 15 px into the third tile column"""
    w, h = request.param, 120
    tiles = _tiles(_grid(oracle, w, h))
    assert tiles[0] == (3, 2), tiles
    five, frames, exp = _case(oracle, w, h)
    ex = _plan(ctx, w, h, len(frames), K)
    yield ex, w, frames, exp
    ex.close()


@pytest.mark.parametrize("pad", [0, 16, 48])
@pytest.mark.parametrize("offset", [0, 1], ids=["in_place", "staged"])
def test_last_window_left_to_the_pitch_clamp(oracle, clamp_plan, pad, offset):
    """row stride = the width rounded up to 16, + pad: read in place, 64 bx + 16 c > pitch - 16 clamps the last one to three
    windows of the last tile column; at offset 1 level 0 is staged into the plan's slab first.  The allocation ends with the
    last frame's last row (tail_unsafe_frame is the last frame of the batch)."""
    ex, w, frames, exp = clamp_plan
    stride = w + (-w) % 16 + pad
    got = _extract_offset(ex, frames, stride, offset)
    _same(got, exp, f"{len(frames)} x {w}x120, stride {stride}, base offset {offset}")
    _pyramid_matches(ex, oracle, frames, f"{w}x120, stride {stride}, base offset {offset}")


# ---------------------------------------------------------------- the advice word
@pytest.mark.parametrize("T", [INI_TH + 1, 45, 255])
def test_forced_threshold(ctx, oracle, T):
    """phase A of every level at T: just above ini_th, a typical advice, and 255 (nothing scores: orb_select redoes every cell)"""
    w, h = 160, 192
    five, frames, exp = _case(oracle, w, h)
    ex = _plan(ctx, w, h, len(frames), K)
    try:
        ex.threshold_hint("forced", T)
        got, _ = _extract(ex, frames, pad=(-w) % 16)
    finally:
        ex.close()
    _same(got, exp, f"{len(frames)} x 160x192, forced T = {T}")


def test_adaptive_sequence_equals_a_plan_with_hints_off(ctx, oracle):
    """textured A, A, the boundary batch B, A (14 x 640x480, 10 x 7 tiles) on one adaptive plan against a plan with hints off and
    the oracle: the first call runs at ini_th, from the second on the word requested with the records carries T > ini_th"""
    fa, fb = np.array(textured_frames(oracle, N_BATCH)), np.array(_batch(oracle))
    ea, eb = _oracle(oracle, fa, K=K_BATCH), _expected(oracle, "batch", K_BATCH)
    assert per_level(N_BATCH, cases.W, cases.H)
    on, off = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH), _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        off.threshold_hint("off")
        above = []
        for i, which in enumerate("AABA"):
            frames, exp = (fa, ea) if which == "A" else (fb, eb)
            above.append(int((on.debug_hints() > INI_TH).sum()))
            got_on, got_off = _extract(on, frames)[0], _extract(off, frames)[0]
            _same(got_on, got_off, f"call {i} ({which}): adaptive against hints off")
            _same(got_on, exp, f"call {i} ({which}): adaptive against the oracle")
        assert above[0] == 0 and above[1] > 0 and above[2] > 0, above
    finally:
        on.close()
        off.close()


# ---------------------------------------------------------------- the other schedules
def test_quadtree_distribution(ctx, oracle):
    """fast_cells_kernel<true>: the score plane of every level through the same prologue"""
    w, h = 160, 192
    five, frames, _ = _case(oracle, w, h)
    ex = _plan(ctx, w, h, len(frames), K)
    try:
        ex.set_distribution(1)
        got, _ = _extract(ex, frames, pad=(-w) % 16)
        _pyramid_matches(ex, oracle, frames, "160x192 quadtree")
    finally:
        ex.close()
    oracle.orb_set_distribution(1)
    try:
        exp5 = _oracle(oracle, five, K=K)
    finally:
        oracle.orb_set_distribution(0)
    idx = np.arange(len(frames)) % len(DISTINCT)
    _same(got, tuple(a[idx] for a in exp5), f"{len(frames)} x 160x192 quadtree")


def test_small_call(ctx, oracle):
    """fast_cells_all_kernel: five frames in one launch for all levels (no magic divisors, no advice, no records)"""
    w, h = 160, 192
    five, _, exp = _case(oracle, w, h)
    assert not per_level(len(five), w, h)
    ex = _plan(ctx, w, h, len(five), K)
    try:
        got, _ = _extract(ex, five, pad=(-w) % 16)
    finally:
        ex.close()
    _same(got, tuple(a[:len(five)] for a in exp), "5 x 160x192 (small)")
