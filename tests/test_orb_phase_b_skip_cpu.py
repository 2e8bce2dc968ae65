"""CPU proof of the phase-B skip of orb_select (gslam_amd/csrc/orb.hip, select_weak_cells), on the oracle alone.

The rule (tests/orb_phase_b_cases.py, skips): if a (level, frame) holds at least quota[l] strong cells -- cells with a strict
3 x 3 maximum of the score map above ini_th -- the cells without one cannot reach the level's output, so orb_select need not
redo them at min_th.  Here the rule is proved against oracle_orb_select_level on every frame that
tests/test_orb_phase_b_skip_gpu.py runs, the frames are shown to hold each case they are meant to hold, and the rule is shown
to hold on the benchmark's frames, which is why the skip fires in the flagship run.  No GPU.
"""
import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_phase_b_cases import INI_TH, K_BATCH, K_STREAM, MIN_TH, frame_census, predictable, select_level, skips, strong_cells, without_weak_cells


@pytest.fixture(scope="module")
def quotas(oracle):
    return oracle.orb_quotas(K_BATCH).tolist()


@pytest.fixture(scope="module")
def batch(oracle, quotas):
    frames = cases.batch_frames(quotas[0])
    return frames, [frame_census(oracle, np.array(f)) for f in frames]


@pytest.fixture(scope="module")
def trap(oracle):
    frames = cases.trap_frames()
    return frames, [frame_census(oracle, np.array(f)) for f in frames[:3]]


@pytest.fixture(scope="module")
def stream(oracle):
    frames = cases.stream_frames()
    return frames, [frame_census(oracle, np.array(f)) for f in frames]


def _marked(c):
    """weak cells with candidates outside flat tiles: what phase A marks and phase B has to redo"""
    return (c["cand"] > 0) & (c["strong_cand"] == 0) & ~c["flat"]


def _prove(oracle, census, quotas, what):
    """-> (skipping pairs, non-skipping pairs); every skipping pair's oracle output survives the loss of its weak cells"""
    n_skip = n_run = 0
    for f, levels in enumerate(census):
        for l, c in enumerate(levels):
            if c is None or quotas[l] <= 0:
                continue
            if not skips(c, quotas[l]):
                n_run += 1
                continue
            n_skip += 1
            full = select_level(oracle, c["S"], INI_TH, quotas[l])
            cut = select_level(oracle, without_weak_cells(c), INI_TH, quotas[l])
            assert len(full) == quotas[l] and np.array_equal(full, cut), (what, f, l, strong_cells(c), quotas[l])
            assert (full[:, 2] > INI_TH).all(), (what, f, l)
    return n_skip, n_run


def test_rule_on_the_boundary_batch(oracle, quotas, batch):
    n_skip, n_run = _prove(oracle, batch[1], quotas, "boundary batch")
    assert n_skip >= 10 and n_run >= 10, (n_skip, n_run)


def test_rule_is_sharp_one_below_the_quota(oracle, quotas, batch):
    """strong = quota - 1 at level 0: the weak cells DO reach the output, a skip there would lose a keypoint"""
    hit = 0
    for (kind, n), levels in zip(cases.batch_kinds(quotas[0]), batch[1]):
        if n != quotas[0] - 1:
            continue
        c = levels[0]
        full = select_level(oracle, c["S"], INI_TH, quotas[0])
        cut = select_level(oracle, without_weak_cells(c), INI_TH, quotas[0])
        assert len(full) == quotas[0] and len(cut) == quotas[0] - 1, (kind, len(full), len(cut))
        hit += 1
    assert hit == 3


def test_rule_on_the_trap_and_the_streamed_frames(oracle, quotas, trap, stream):
    _prove(oracle, trap[1], quotas, "trap")
    n_skip, n_run = _prove(oracle, stream[1], oracle.orb_quotas(K_STREAM).tolist(), "2560x1440")
    assert n_skip >= 1 and n_run >= 1


def test_batch_holds_every_case(oracle, quotas, batch):
    q0 = quotas[0]
    assert 24 <= q0 <= 48, quotas  # "a few dozen"
    frames, census = batch
    assert len(frames) == cases.N_BATCH and frames.shape[1:] == (cases.H, cases.W)
    seen0, upper = set(), set()
    dense = capped = 0
    for (kind, n), levels in zip(cases.batch_kinds(q0), census):
        c = levels[0]
        if n is not None:
            assert strong_cells(c) == n, (kind, n, strong_cells(c))
            # identical strong corners in distinct cells: one candidate of score 100 per strong cell
            assert (c["strong_cand"] <= 1).all() and set(np.unique(c["S"][c["S"] > INI_TH]).tolist()) == {100}
            # every weak dot sits in a tile that is not flat at ini_th: it reaches phase B, not the flat-tile shortcut
            weak = (c["cand"] > 0) & (c["strong_cand"] == 0)
            assert weak.sum() >= n // 2 and not (weak & c["flat"]).any(), kind
            dense += int((_marked(c) & (c["nz"] > 64)).sum())
            capped += int((_marked(c) & (c["cand"] > 32)).sum())
        seen0.add(int(np.sign(strong_cells(c) - q0)) if abs(strong_cells(c) - q0) <= 1 else None)
        for l, cl in enumerate(levels):
            assert predictable(cl, quotas[l]), (kind, l)
            if l >= 1 and cl is not None and quotas[l] > 0:
                upper.add((skips(cl, quotas[l]), bool(_marked(cl).any())))
    assert {-1, 0, 1} <= seen0, seen0
    assert dense >= 9 and capped >= 9, (dense, capped)
    # a level >= 1 that skips while it holds marked cells with candidates, and one that does not skip and holds some
    assert (True, True) in upper and (False, True) in upper, upper
    # the skip also leaves marked cells with more than 64 scored pixels / more than 32 candidates behind (weak_region: 56 >= q0)
    c = census[[k for k, _ in cases.batch_kinds(q0)].index("weak_region")][0]
    assert skips(c, q0) and (_marked(c) & (c["nz"] > 64)).sum() > 20 and (_marked(c) & (c["cand"] > 32)).sum() > 20
    c = census[[k for k, _ in cases.batch_kinds(q0)].index("weak_region_short")][0]
    assert not skips(c, q0) and strong_cells(c) == 28


def test_trap_frames_hold_the_trap(oracle, quotas, trap):
    q0 = quotas[0]
    for levels in trap[1]:
        c = levels[0]
        strong = strong_cells(c)
        flat_cells = (c["cand"] > 0) & c["flat"]                 # finished single-phase by orb_fast_cells: ordinary counts, weak scores
        assert strong < q0 <= strong + flat_cells.sum(), (strong, q0, int(flat_cells.sum()))
        assert _marked(c).sum() >= 10 and (c["strong_cand"][flat_cells] == 0).all()
        assert all(predictable(cl, quotas[l]) for l, cl in enumerate(levels))
        # a count without the score test skips: the marked cells' records then read as empty, and the output changes
        full = select_level(oracle, c["S"], INI_TH, q0)
        lost = select_level(oracle, without_weak_cells(c, keep=c["flat"]), INI_TH, q0)
        assert len(full) == q0 and len(lost) == q0 and not np.array_equal(full, lost)


def test_streamed_frames_need_both_rounds(oracle, stream):
    q0 = int(oracle.orb_quotas(K_STREAM)[0])
    quotas = oracle.orb_quotas(K_STREAM).tolist()
    (c0, c1) = (levels[0] for levels in stream[1])
    assert c0["ncx"] * c0["ncy"] == 3476
    s = (c0["strong_cand"] > 0).reshape(-1)
    assert s[:2048].sum() < q0 and s[2048:].sum() < q0 and s.sum() >= q0, (int(s[:2048].sum()), int(s[2048:].sum()), q0)
    assert _marked(c0).reshape(-1)[:2048].sum() > 100  # the skip leaves marked cells behind
    assert not skips(c1, q0) and _marked(c1).reshape(-1)[:2048].sum() > 100 and _marked(c1).reshape(-1)[2048:].sum() > 100
    for levels in stream[1]:
        assert all(predictable(cl, quotas[l]) for l, cl in enumerate(levels))


def test_rule_holds_on_the_benchmark_frames(oracle):
    """bench.py's frames, 1920x1080, K = 2000: every level of frames 0 and 999 holds more strong cells than its quota -- phase B
    never runs in the flagship step.  The tightest level is the last one."""
    quotas = oracle.orb_quotas(2000).tolist()
    assert quotas == [434, 362, 302, 251, 209, 175, 145, 122]
    for f in (0, 999):
        levels = frame_census(oracle, oracle.synth_frame(1920, 1080, 0x5EED0000 + f))
        for l, c in enumerate(levels):
            assert skips(c, quotas[l]), (f, l, strong_cells(c), quotas[l])
        assert strong_cells(levels[7]) - quotas[7] > 0
        assert levels[7]["ncx"] * levels[7]["ncy"] == 144 and levels[0]["ncx"] * levels[0]["ncy"] == 1947


def test_existing_counter_batch_still_runs_phase_b(oracle):
    """tests/test_orb_two_phase_gpu.py::test_counters asserts weak_cells, dense_cells, cap_cells, rank_dropped and overflow_cells
    > 0 on its batch (K = 1000): its (level, frame) pairs that do not skip still send cells with candidates, with more than 64
    scored pixels and with more than 32 candidates through phase B."""
    import test_orb_two_phase_gpu as two
    quotas = oracle.orb_quotas(1000).tolist()
    weak = dense = capped = 0
    for f in two._frames(two.N_PER_LEVEL)[:7]:
        for l, c in enumerate(frame_census(oracle, np.array(f))):
            if c is None or quotas[l] <= 0 or skips(c, quotas[l]):
                continue
            m = _marked(c)
            weak, dense, capped = weak + int(m.sum()), dense + int((m & (c["nz"] > 64)).sum()), capped + int((m & (c["cand"] > 32)).sum())
    assert weak > 0 and dense > 0 and capped > 0, (weak, dense, capped)
