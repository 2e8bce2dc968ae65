"""GPU parity of the quantised pass 1 of orb_fast_cells (gslam_amd/csrc/orb.hip: fast_compass4_q, fast_cells_tile).

Phase A of the two-phase detector at T > ini_th queues the pixels that pass a conservative compass test on 6-bit pixels; pass 2
scores them exactly, so every output must stay what it was.  Forced T (gh_orb_plan_set_threshold_hint) on the per-level path,
bit for bit against oracle.orb_extract_batch: counts, all 28 keypoint bytes, descriptors, the zero tail.
tests/test_orb_pass1_quant_cpu.py proves the arithmetic; here the kernel runs it on frames built to sit on the quantisation
edges, in interior, last-column and first / last-row tiles.
"""
import functools

import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_phase_b_cases import INI_TH, K_BATCH, N_BATCH
from orb_threshold_hint_cases import textured_frames
from test_orb_per_level_gpu import _extract, _oracle, _plan, _same, overlap, per_level
from test_orb_phase_b_skip_gpu import _batch, _expected

pytestmark = pytest.mark.gpu

K = 2000
# every residue of T + 1 mod 4 twice (t' steps at 23, 27, 43 ...), and the clamp: t' = 63 at 252 and 254, 64 at 255
FORCED = (21, 22, 23, 24, 26, 27, 43, 252, 254, 255)
EW, EH = 256, 192   # 7 x 5 cells: 4 x 3 tiles, the last tile column half empty
N_EDGE = 87         # the smallest multiple of three frames on the per-level path


def edge_texture(T, seed):
    """(a) 16 x 16 patches of a flat background b with an isolated pixel, a 3 x 3 and a 5 x 5 block at b + (T + e) or b - (T + e),
    e in {0, 1, 3, 4}: the exact test passes from e = 1 on, the quantised one depends on b mod 4.  b runs through eight
    consecutive values, so every alignment to a multiple of 4 occurs with every e and both signs."""
    rng = np.random.default_rng(seed)
    img = np.zeros((EH, EW), np.int32)
    n = 0
    for y in range(0, EH, 16):
        for x in range(0, EW, 16):
            e, sign, r = (0, 1, 3, 4)[n % 4], (1, -1)[(n // 4) % 2], (n // 8) % 8
            room = max(0, 255 - 7 - (T + 4))
            lift = 8 * int(rng.integers(0, room // 8 + 1))
            b = r + lift if sign > 0 else 255 - r - lift
            v = min(255, max(0, b + sign * (T + e)))
            img[y:y + 16, x:x + 16] = b
            img[y + 3, x + 3] = v
            img[y + 9:y + 12, x + 2:x + 5] = v
            img[y + 5:y + 10, x + 8:x + 13] = v
            n += 1
    return img.astype(np.uint8)


def edge_blocks(seed):
    """(b) blocks of 255 on 0 (left half) and of 0 on 255 (right half), 1 .. 6 px wide: q differs by 63, the carry bound at t' = 64"""
    rng = np.random.default_rng(seed)
    img = np.zeros((EH, EW), np.uint8)
    img[:, EW // 2:] = 255
    for y in range(2, EH - 8, 9):
        for x in range(2, EW - 8, 9):
            s = int(rng.integers(1, 7))
            img[y:y + s, x:x + s] = 255 if x < EW // 2 else 0
    return img


def edge_frames(T):
    """the three frames, cycled to the smallest batch that takes the per-level path"""
    three = np.stack([edge_texture(T, 100 + T), edge_blocks(200 + T),
                      np.random.default_rng(300 + T).integers(0, 256, (EH, EW), dtype=np.uint8)])
    return three, np.stack([three[i % 3] for i in range(N_EDGE)])


def _cycled(exp3, n):
    return tuple(np.stack([a[i % 3] for i in range(n)]) for a in exp3)


@functools.lru_cache(maxsize=None)
def _boundary(oracle):
    frames = np.array(_batch(oracle))
    return frames, _oracle(oracle, frames, K=K)


@functools.lru_cache(maxsize=None)
def _textured(oracle):
    frames = np.array(textured_frames(oracle, N_BATCH))
    return frames, _oracle(oracle, frames, K=K)


@pytest.fixture(scope="module")
def batch_plan(ctx):
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K)
    yield ex
    ex.close()


@pytest.fixture(scope="module")
def edge_plan(ctx):
    ex = _plan(ctx, EW, EH, N_EDGE, K)
    yield ex
    ex.close()


@pytest.mark.parametrize("T", FORCED)
def test_forced_threshold_on_the_boundary_batch(oracle, batch_plan, T):
    """14 x 640x480 at K = 2000: flat, weak and exactly-at-the-quota frames"""
    assert per_level(N_BATCH, cases.W, cases.H) and not overlap(N_BATCH, cases.W, cases.H)
    frames, exp = _boundary(oracle)
    batch_plan.threshold_hint("forced", T)
    try:
        _same(_extract(batch_plan, frames)[0], exp, f"boundary batch, forced T = {T}")
    finally:
        batch_plan.threshold_hint("adaptive")


@pytest.mark.parametrize("T", FORCED)
def test_forced_threshold_on_the_quantisation_edges(oracle, edge_plan, T):
    """87 x 256x192: differences of exactly T, T + 1, T + 3, T + 4 around multiples of 4; 255 against 0; full-range noise"""
    assert per_level(N_EDGE, EW, EH) and not per_level(N_EDGE - 3, EW, EH)
    three, frames = edge_frames(T)
    exp = _cycled(_oracle(oracle, three, K=K), N_EDGE)
    edge_plan.threshold_hint("forced", T)
    try:
        _same(_extract(edge_plan, frames)[0], exp, f"quantisation edges, forced T = {T}")
    finally:
        edge_plan.threshold_hint("adaptive")


def test_adaptive_sequence_equals_a_plan_with_hints_off(ctx, oracle):
    """textured A, A, the boundary batch B, A on one adaptive plan against the same calls on a plan with hints off (and the
    oracle): from the second call on the adaptive plan runs levels above ini_th, on the quantised pass 1"""
    # (K = 150 as in tests/test_orb_threshold_hint_gpu.py: at K = 2000 quota[0] exceeds the cells of level 0, the cut never
    # falls in rank 0 and no advice rises)
    fa, fb = np.array(textured_frames(oracle, N_BATCH)), np.array(_batch(oracle))
    ea, eb = _oracle(oracle, fa, K=K_BATCH), _expected(oracle, "batch", K_BATCH)
    on, off = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH), _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        off.threshold_hint("off")
        above = []  # (slot, level) pairs that the call runs above ini_th
        for i, which in enumerate("AABA"):
            frames, exp = (fa, ea) if which == "A" else (fb, eb)
            above.append(int((on.debug_hints() > INI_TH).sum()))
            got_on, got_off = _extract(on, frames)[0], _extract(off, frames)[0]
            _same(got_on, got_off, f"call {i} ({which}): adaptive against hints off")
            _same(got_on, exp, f"call {i} ({which}): adaptive against the oracle")
        print("(slot, level) pairs above ini_th going into each call:", above)
        assert above[0] == 0 and above[1] > 0 and above[2] > 0, above
        assert (off.debug_hints() == INI_TH).all()
    finally:
        on.close()
        off.close()


def test_exact_pass1_stays_where_it_was(ctx, oracle, batch_plan):
    """the dispatch: forced T == ini_th and hints off run the exact test (same census, the flat-tile shortcut included); a small
    call and the quadtree mode are single-phase and ignore the advice"""
    frames, exp = _boundary(oracle)
    census = {}
    for mode, T in (("off", 0), ("forced", INI_TH)):
        batch_plan.threshold_hint(mode, T)
        try:
            got, d = _extract(batch_plan, frames, counters=True)
        finally:
            batch_plan.threshold_hint("adaptive")
        _same(got, exp, f"boundary batch, {mode} {T}, counters on")
        census[mode] = d
    assert census["off"] == census["forced"], census
    assert census["off"]["max_queue"] > 0 and census["off"]["weak_cells"] > 0, census

    fa, ea = _textured(oracle)
    ex = _plan(ctx, cases.W, cases.H, 1, K)
    try:
        assert not per_level(1, cases.W, cases.H)
        ex.threshold_hint("forced", 43)
        _same(_extract(ex, fa[:1])[0], tuple(a[:1] for a in ea), "1 x 640x480 (one launch for all levels), forced 43")
    finally:
        ex.close()
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        ex.set_distribution(1)
        plain, _ = _extract(ex, fa)
        ex.threshold_hint("forced", 43)
        forced, _ = _extract(ex, fa)
        _same(forced, (np.ascontiguousarray(plain[0]).view(np.uint8).reshape(N_BATCH, K_BATCH, 28), plain[1], plain[2]), "quadtree, forced 43")
        oracle.orb_set_distribution(1)
        try:
            ek, ed = oracle.orb_extract(fa[0], K_BATCH)
        finally:
            oracle.orb_set_distribution(0)
        gk = np.ascontiguousarray(forced[0]).view(np.uint8).reshape(N_BATCH, K_BATCH, 28)
        assert forced[2][0] == len(ek) and gk[0, :len(ek)].tobytes() == ek.tobytes() and np.array_equal(forced[1][0, :len(ek)], ed)
    finally:
        ex.close()
