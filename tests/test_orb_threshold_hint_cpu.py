"""CPU proof of the threshold hint of large ORB calls (gslam_amd/csrc/orb.hip: fast_cells_tile, select_weak_cells), on the
oracle alone.

Phase A at T >= ini_th stores the scores above T only, so a cell's record holds its candidates above T with their true ranks.
The rule (tests/orb_threshold_hint_cases.py): if at least quota[l] cells of a (level, frame) hold a candidate above T, the
selection from those cut records is the oracle's; with fewer, it need not be, and the level is redone.  Proved here with
oracle_orb_select_level on the score map cut at T, for T in {ini_th, 21, 36, 60, 120}, on every level of the boundary batch of
tests/orb_phase_b_cases.py and of two textured frames.  No GPU.
"""
import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_phase_b_cases import INI_TH, K_BATCH, select_level
from orb_threshold_hint_cases import (HintModel, cut_at, cut_score, frame_cells, hint_from_cut, hint_next, premise, t_strong_cells,
                                      textured_frames)

THRESHOLDS = (INI_TH, 21, 36, 60, 120)
K_TEXTURED = 300


@pytest.fixture(scope="module")
def quotas(oracle):
    return oracle.orb_quotas(K_BATCH).tolist()


@pytest.fixture(scope="module")
def batch(oracle, quotas):
    return [frame_cells(oracle, f) for f in cases.batch_frames(quotas[0])]


@pytest.fixture(scope="module")
def textured(oracle):
    return [frame_cells(oracle, f) for f in textured_frames(oracle, 2)]


def _prove(oracle, census, quotas, what):
    """-> {T: [pairs where the premise holds, pairs where it does not]}; wherever it holds, the cut records select what the
    complete ones do"""
    seen = {T: [0, 0] for T in THRESHOLDS}
    for f, levels in enumerate(census):
        for l, c in enumerate(levels):
            if c is None or quotas[l] <= 0:
                continue
            full = select_level(oracle, c["S"], INI_TH, quotas[l])
            for T in THRESHOLDS:
                if not premise(c, quotas[l], T):
                    seen[T][1] += 1
                    continue
                seen[T][0] += 1
                # (the filter of oracle step 4 at T keeps every entry of the cut map: all of them score above T)
                cut = select_level(oracle, cut_at(c, T), T, quotas[l])
                assert len(full) == quotas[l] and np.array_equal(full, cut), (what, f, l, T, t_strong_cells(c, T), quotas[l])
                assert (full[:, 2] > T).all(), (what, f, l, T)
    return seen


def test_rule_on_the_boundary_batch(oracle, quotas, batch):
    seen = _prove(oracle, batch, quotas, "boundary batch")
    print(seen)
    for T in (INI_TH, 21, 36, 60):
        assert seen[T][0] >= 5 and seen[T][1] >= 5, seen
    assert seen[120][1] >= 50, seen  # (the strong corners of the batch score 100 at most)


def test_rule_on_textured_frames(oracle, textured):
    quotas = oracle.orb_quotas(K_TEXTURED).tolist()
    seen = _prove(oracle, textured, quotas, "textured")
    print(seen)
    assert seen[INI_TH][0] >= 8 and seen[36][0] >= 8, seen
    assert sum(v[1] for v in seen.values()) >= 1, seen


def test_one_cell_short_fails_the_premise_and_the_cut_records(oracle, quotas, batch):
    """level 0 of the frames with quota - 1 strong cells (every strong corner scores 100): the premise fails at every T below 100,
    and there the cut records DO select something else -- they lack the weak cells' entries that fill the quota"""
    q0, hit = quotas[0], 0
    for (kind, n), levels in zip(cases.batch_kinds(q0), batch):
        c = levels[0]
        for T in (INI_TH, 21, 36, 60):
            if n is not None:
                assert t_strong_cells(c, T) == n, (kind, T)
            if n != q0 - 1:
                continue
            assert not premise(c, q0, T)
            full = select_level(oracle, c["S"], INI_TH, q0)
            cut = select_level(oracle, cut_at(c, T), T, q0)
            assert len(full) == q0 and len(cut) == q0 - 1, (kind, T, len(full), len(cut))
            hit += 1
    assert hit == 3 * 4


def test_premise_holds_at_the_cut_derived_threshold(oracle, quotas, batch, textured):
    """T from a frame's own cut (hint_from_cut) lies below s*, so the same frame satisfies the premise at it: a repeated frame
    never mispredicts"""
    rose = 0
    for census, qs in ((batch, quotas), (textured, oracle.orb_quotas(K_TEXTURED).tolist())):
        for levels in census:
            for l, c in enumerate(levels):
                if c is None or qs[l] <= 0:
                    continue
                s = cut_score(c, qs[l])
                T = hint_from_cut(s)
                assert INI_TH <= T <= 255
                if T > INI_TH:
                    rose += 1
                    assert T < s and premise(c, qs[l], T), (l, s, T)
    assert rose >= 10, rose


def test_hold_off_bounds_mispredictions():
    """hint_next alone, on a slot that mispredicts whenever it runs above ini_th: the holds double up to 64 calls, so at most one
    redo in 66 calls from then on (hint_threshold, which lets a slot with a penalty up in every other call only, can add one);
    calls that hold above ini_th take the penalty down again"""
    state, redo = (INI_TH, 0, 0), []
    for call in range(1000):
        mis = state[0] > INI_TH
        if mis:
            redo.append(call)
        state = hint_next(state, 80, mis)
    gaps = np.diff(redo)
    assert gaps[:6].tolist() == [4, 6, 10, 18, 34, 66] and (gaps[5:] == 66).all(), gaps[:10]
    for _ in range(200):
        state = hint_next(state, 80, False)
    assert state == (hint_from_cut(80), 0, 0) and state[0] == 60, state


def test_model_drives_every_slot_and_level(oracle, quotas, batch, textured):
    m = HintModel(2, oracle.orb_quotas(K_TEXTURED).tolist())
    m.call(textured)
    assert (m.hints() > INI_TH).any() and not m.mispredicted
    m.call(textured)
    assert not m.mispredicted
