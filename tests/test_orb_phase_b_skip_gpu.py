"""GPU parity of the phase-B skip of orb_select (gslam_amd/csrc/orb.hip, select_weak_cells).

Where the two-phase detector runs, the workgroup of a (level, frame) counts the level's strong cells and redoes the cells that
phase A marked only if that count is below the level's quota; after a skip the marks stay and read as empty cells.  The
frames (tests/orb_phase_b_cases.py; tests/test_orb_phase_b_skip_cpu.py proves the rule on them and shows that they hold each
case) put the count one below, at and one above the quota.  A wrong skip loses keypoints, so every output is compared bit for
bit with oracle.orb_extract_batch -- counts, all 28 keypoint bytes, descriptors, the zero tail -- as in
tests/test_orb_two_phase_gpu.py.  A missing skip shows only in the weak_cells debug counter (cells with candidates and no strong
one that some kernel processed at min_th), which must equal the CPU census exactly.
"""
import functools

import numpy as np
import pytest

import orb_phase_b_cases as cases
from orb_phase_b_cases import K_BATCH, K_STREAM, N_BATCH, frame_census, predicted_weak_cells, skips
from test_orb_per_level_gpu import _gpu, _oracle, _same, overlap, per_level

pytestmark = pytest.mark.gpu

N_OVERLAP = 55


@functools.lru_cache(maxsize=None)
def _batch(oracle):
    return cases.batch_frames(int(oracle.orb_quotas(K_BATCH)[0]))


@functools.lru_cache(maxsize=None)
def _expected(oracle, which, K, ini_th=20, min_th=7):
    frames = {"batch": lambda: _batch(oracle), "trap": cases.trap_frames, "stream": cases.stream_frames,
              "overlap": lambda: _overlap_frames(oracle)}[which]()
    return _oracle(oracle, np.array(frames), K=K, ini_th=ini_th, min_th=min_th)


def _overlap_frames(oracle):
    b = _batch(oracle)
    return np.stack([b[i % N_BATCH] for i in range(N_OVERLAP)])


def _predicted(oracle, frames, K):
    quotas = oracle.orb_quotas(K).tolist()
    return sum(predicted_weak_cells(c, quotas[l]) for f in frames for l, c in enumerate(frame_census(oracle, np.array(f))))


def test_boundary_batch(ctx, oracle):
    """14 x 640x480, K = 150 (quota[0] = 33): level 0 holds 32, 33 and 34 strong cells, upper levels skip and do not skip."""
    frames = np.array(_batch(oracle))
    assert per_level(N_BATCH, cases.W, cases.H) and not overlap(N_BATCH, cases.W, cases.H)
    got, _ = _gpu(ctx, frames, K=K_BATCH)
    _same(got, _expected(oracle, "batch", K_BATCH), "boundary batch")
    got, d = _gpu(ctx, frames, K=K_BATCH, counters=True)
    _same(got, _expected(oracle, "batch", K_BATCH), "boundary batch, counters on")
    want = _predicted(oracle, frames, K_BATCH)
    print("weak_cells", d["weak_cells"], "census", want)
    assert d["weak_cells"] == want, (d, want)


def test_flat_tile_trap(ctx, oracle):
    """strong < quota <= strong + the non-empty cells of flat tiles, which carry ordinary counts: a count that ignores the
    score test skips here and loses the marked cells' keypoints."""
    frames = np.array(cases.trap_frames())
    got, d = _gpu(ctx, frames, K=K_BATCH, counters=True)
    _same(got, _expected(oracle, "trap", K_BATCH), "flat-tile trap")
    want = _predicted(oracle, frames, K_BATCH)
    print("weak_cells", d["weak_cells"], "census", want)
    assert d["weak_cells"] == want, (d, want)


def test_several_gathering_rounds(ctx, oracle):
    """2 x 2560x1440, K = 8000: level 0 has 3476 cells, the streaming select gathers in two rounds and counts in a pass of its
    own in front of them.  Frame 0 reaches quota[0] only with the cells of both rounds; frame 1 stays short."""
    frames = np.array(cases.stream_frames())
    assert per_level(2, 2560, 1440)
    got, d = _gpu(ctx, frames, K=K_STREAM, counters=True)
    _same(got, _expected(oracle, "stream", K_STREAM), "2 x 2560x1440")
    assert d["sel_streamed"] > 0, d
    want = _predicted(oracle, frames, K_STREAM)
    print("weak_cells", d["weak_cells"], "census", want)
    assert d["weak_cells"] == want, (d, want)


def test_overlap_schedule(ctx, oracle):
    """55 x 640x480: select(l), with its count and skip, runs on the side stream beside fast_cells(l + 1)."""
    assert overlap(N_OVERLAP, cases.W, cases.H)
    got, _ = _gpu(ctx, _overlap_frames(oracle), K=K_BATCH)
    _same(got, _expected(oracle, "overlap", K_BATCH), "overlap schedule")


@pytest.mark.parametrize("th", [(254, 1), (9, 8)], ids=["ini254-min1", "ini9-min8"])
def test_other_thresholds(ctx, oracle, th):
    """(254, 1): nearly everything is weak and nothing skips; (9, 8): the weak dots of the batch (score 12) are strong."""
    ini_th, min_th = th
    frames = np.array(_batch(oracle))
    if ini_th == 254:
        quotas = oracle.orb_quotas(K_BATCH).tolist()
        assert not any(skips(c, quotas[l]) for f in frames[:3] for l, c in enumerate(frame_census(oracle, f, ini_th=ini_th, min_th=min_th))
                       if c is not None)
    got, _ = _gpu(ctx, frames, K=K_BATCH, ini_th=ini_th, min_th=min_th)
    _same(got, _expected(oracle, "batch", K_BATCH, ini_th, min_th), f"ini_th={ini_th} min_th={min_th}")
