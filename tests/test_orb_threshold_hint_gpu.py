"""GPU parity of the threshold hint of large ORB calls (gslam_amd/csrc/orb.hip: fast_cells_tile, select_weak_cells, hint_next).

Phase A of the two-phase detector may run a (level, frame) at any T >= ini_th; orb_select redoes the whole level where fewer
than quota[l] cells hold a corner above T.  T is advice: every output here is compared bit for bit with
oracle.orb_extract_batch -- counts, all 28 keypoint bytes, descriptors, the zero tail -- whatever T was forced or learnt, and
the learnt T of every (slot, level) must equal the Python restatement of the update rule on the CPU census
(tests/orb_threshold_hint_cases.py; tests/test_orb_threshold_hint_cpu.py proves the rule itself).
"""
import functools

import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_phase_b_cases import INI_TH, K_BATCH, K_STREAM, N_BATCH
from orb_threshold_hint_cases import HintModel, frame_cells, textured_frames
from test_orb_per_level_gpu import _extract, _frames, _oracle, _plan, _same, overlap, per_level
from test_orb_phase_b_skip_gpu import N_OVERLAP, _batch, _expected, _overlap_frames

pytestmark = pytest.mark.gpu

FORCED = (20, 21, 36, 60, 120, 254, 255)
K_MIXED = 2000


@functools.lru_cache(maxsize=None)
def _mixed(oracle):
    """every image class, K = 2000: quota[0] = 434 exceeds the 266 cells of level 0, so entries of rank >= 1 decide"""
    frames = _frames(640, 480, N_BATCH)
    return frames, _oracle(oracle, frames, K=K_MIXED)


@functools.lru_cache(maxsize=None)
def _textured(oracle):
    frames = np.array(textured_frames(oracle, N_BATCH))
    return frames, _oracle(oracle, frames, K=K_BATCH)


@functools.lru_cache(maxsize=None)
def _census(oracle, which):
    frames = {"textured": lambda: _textured(oracle)[0], "batch": lambda: _batch(oracle)}[which]()
    return [frame_cells(oracle, f) for f in frames]


@pytest.mark.parametrize("which", ["boundary", "mixed"])
def test_forced_advice_is_invisible(ctx, oracle, which):
    """14 x 640x480, the smallest per-level batch.  255 sends every level through the redo of all its cells; 254 keeps the
    corners of score 255 alone."""
    assert per_level(N_BATCH, cases.W, cases.H)
    if which == "boundary":
        frames, K, exp = np.array(_batch(oracle)), K_BATCH, _expected(oracle, "batch", K_BATCH)
    else:
        (frames, exp), K = _mixed(oracle), K_MIXED
        assert int(oracle.orb_quotas(K)[0]) == 434
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K)
    try:
        for T in FORCED:
            ex.threshold_hint("forced", T)
            got, _ = _extract(ex, frames)
            _same(got, exp, f"{which}, forced T = {T}")
        assert (ex.debug_hints() == INI_TH).all()  # nothing is updated while forced
        ex.threshold_hint("off")
        got, _ = _extract(ex, frames)
        _same(got, exp, f"{which}, hints off")
        assert (ex.debug_hints() == INI_TH).all()
    finally:
        ex.close()


@pytest.mark.parametrize("th", [(9, 8), (254, 1)], ids=["ini9-min8", "ini254-min1"])
def test_forced_advice_is_clamped_to_ini_th(ctx, oracle, th):
    ini_th, min_th = th
    frames = np.array(_batch(oracle))
    exp = _expected(oracle, "batch", K_BATCH, ini_th, min_th)
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH, ini_th=ini_th, min_th=min_th)
    try:
        for T in (0, 100):
            ex.threshold_hint("forced", T)
            got, _ = _extract(ex, frames)
            _same(got, exp, f"ini_th={ini_th} min_th={min_th}, forced T = {T}")
    finally:
        ex.close()


def test_adaptive_sequence_on_one_plan(ctx, oracle):
    """textured A, A, A, the boundary batch B (flat, weak and exactly-at-the-quota frames), B, then A, A on ONE plan: every call
    equals the oracle, and after every call the plan's T of every (slot, level) is what the update rule gives on the census"""
    (fa, ea), (fb, eb) = _textured(oracle), (np.array(_batch(oracle)), _expected(oracle, "batch", K_BATCH))
    quotas = oracle.orb_quotas(K_BATCH).tolist()
    model = HintModel(N_BATCH, quotas)
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        assert (ex.debug_hints() == INI_TH).all()
        rose = False
        for i, which in enumerate("AAABBAA"):
            frames, exp = (fa, ea) if which == "A" else (fb, eb)
            got, _ = _extract(ex, frames)
            _same(got, exp, f"call {i} ({which})")
            model.call(_census(oracle, "textured" if which == "A" else "batch"))
            hints = ex.debug_hints()
            bad = np.argwhere(hints != model.hints())
            assert len(bad) == 0, (i, which, bad[:5].tolist(), hints[bad[0][0]].tolist(), model.hints()[bad[0][0]].tolist())
            if i == 2:
                rose = bool((hints > INI_TH).any())
                assert not model.mispredicted
        assert rose
        print("mispredicted (call, slot, level):", model.mispredicted)
        assert any(c == 3 for c, _, _ in model.mispredicted), model.mispredicted
    finally:
        ex.close()


def test_debug_counters_see_the_call_at_ini_th(ctx, oracle):
    """while the branch census is on, adaptive advice is neither applied nor updated"""
    fa, ea = _textured(oracle)
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        got, d = _extract(ex, fa, counters=True)
        _same(got, ea, "counters on")
        assert (ex.debug_hints() == INI_TH).all() and d["cells"] > 0
    finally:
        ex.close()


def test_streaming_select(ctx, oracle):
    """2 x 2560x1440, K = 8000: level 0 gathers in two rounds; forced 60, then adaptive over two calls"""
    frames, exp = np.array(cases.stream_frames()), _expected(oracle, "stream", K_STREAM)
    assert per_level(2, 2560, 1440)
    ex = _plan(ctx, 2560, 1440, 2, K_STREAM)
    try:
        ex.threshold_hint("forced", 60)
        _same(_extract(ex, frames)[0], exp, "2 x 2560x1440, forced 60")
        ex.threshold_hint("forced", 255)
        _same(_extract(ex, frames)[0], exp, "2 x 2560x1440, forced 255")
        ex.threshold_hint("adaptive")
        for i in range(2):
            _same(_extract(ex, frames)[0], exp, f"2 x 2560x1440, adaptive call {i}")
        print("hints", ex.debug_hints().tolist())
    finally:
        ex.close()


def test_overlap_schedule(ctx, oracle):
    """55 x 640x480: select(l) reads and writes the advice on the side stream beside fast_cells(l + 1)"""
    assert overlap(N_OVERLAP, cases.W, cases.H)
    frames, exp = _overlap_frames(oracle), _expected(oracle, "overlap", K_BATCH)
    ex = _plan(ctx, cases.W, cases.H, N_OVERLAP, K_BATCH)
    try:
        for i in range(3):
            _same(_extract(ex, frames)[0], exp, f"overlap, adaptive call {i}")
        assert (ex.debug_hints() > INI_TH).any()
        ex.threshold_hint("forced", 60)
        _same(_extract(ex, frames)[0], exp, "overlap, forced 60")
    finally:
        ex.close()


def test_ignored_where_single_phase(ctx, oracle):
    """a small call (one launch for all levels) and the quadtree mode are single-phase: forced advice changes nothing, the
    plan's advice stays untouched"""
    import torch
    from gslam_amd.orb import kps_to_numpy
    frames, exp = _textured(oracle)
    ex = _plan(ctx, cases.W, cases.H, 1, K_BATCH)
    try:
        assert not per_level(1, cases.W, cases.H)
        ex.threshold_hint("forced", 100)
        _same(_extract(ex, frames[:1])[0], tuple(a[:1] for a in exp), "1 x 640x480, forced 100")
        ex.threshold_hint("adaptive")
        _same(_extract(ex, frames[:1])[0], tuple(a[:1] for a in exp), "1 x 640x480, adaptive")
        assert (ex.debug_hints() == INI_TH).all()
    finally:
        ex.close()
    ex = _plan(ctx, cases.W, cases.H, N_BATCH, K_BATCH)
    try:
        ex.set_distribution(1)
        plain, _ = _extract(ex, frames)
        ex.threshold_hint("forced", 100)
        forced, _ = _extract(ex, frames)
        _same(forced, (np.ascontiguousarray(plain[0]).view(np.uint8).reshape(N_BATCH, K_BATCH, 28), plain[1], plain[2]), "quadtree, forced 100")
        assert (ex.debug_hints() == INI_TH).all()
        oracle.orb_set_distribution(1)
        try:
            ek, ed = oracle.orb_extract(frames[0], K_BATCH)
        finally:
            oracle.orb_set_distribution(0)
        kp = kps_to_numpy(torch.from_numpy(forced[0]))
        assert forced[2][0] == len(ek) and kp[0, :len(ek)].tobytes() == ek.tobytes() and np.array_equal(forced[1][0, :len(ek)], ed)
    finally:
        ex.close()
