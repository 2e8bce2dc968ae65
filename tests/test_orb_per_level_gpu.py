"""Adversarial GPU parity of the ORB front end on the per-level path of gh_orb_extract_dev, the path of large calls.

Which code runs depends only on the call's pixel count, batch * w * h (gslam_amd/csrc/orb.hip, orb_schedule; the launch
counts of each schedule are pinned by tests/test_orb_schedule_gpu.py):
  <= 4 << 20   small: the whole pyramid by the stand-alone resize, every level in one fast_cells_all_kernel launch, one
               select; a captured graph replays the call
  >  4 << 20   per-level: one fast_cells_kernel<false> launch per level, each building the next pyramid level inside
               the kernel (MFMA on interior tiles, VALU on edge tiles, split by own_gx / own_gy); a level with quota 0 or
               no cells gets the stand-alone resize instead
  >= 16 << 20  per-level, and select runs per level on a side stream joined by events (overlap)
  and any level of more than kSelCached * 256 = 2048 cells takes the streaming select_kernel<false>.
tests/test_orb_adversarial_gpu.py holds the small path to the oracle on the same image classes; this file does the same
for the per-level path, in the production configuration (debug counters off) except in the census.  Every comparison is
bit-exact on all 28 + 32 bytes of every record, the counts and the zero tail, against
oracle.orb_extract_batch (oracle/orb_oracle.c).
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from ba_parity import THREADS
from orb_images import CLASSES

pytestmark = pytest.mark.gpu

NAMES = sorted(CLASSES)
# the dispatch thresholds of orb.hip (orb_schedule): kAllLevelsMaxPx and kOverlapMinPx
SMALL_MAX_PX = 4 << 20
OVERLAP_MIN_PX = 16 << 20
SEL_CACHED_CELLS = 8 * 256  # orb.hip kSelCachedMaxCells = kSelCached * 256: larger levels take the streaming select


def per_level(batch, w, h):
    return batch * w * h > SMALL_MAX_PX


def overlap(batch, w, h):
    return batch * w * h >= OVERLAP_MIN_PX


def first_per_level(w, h):
    return SMALL_MAX_PX // (w * h) + 1


def _frames(w, h, n, offset=0, seed=1000):
    """n frames cycling through all image classes from `offset`, each with its own seed (frame i does not depend on n)."""
    return np.stack([CLASSES[NAMES[(offset + i) % len(NAMES)]](w, h, seed + 7919 * i) for i in range(n)])


def _grid(oracle, w, h, nlevels=8):
    """(ncx, ncy) of every level, as gh_orb_plan_create computes them (19-px border, 32-px cells)."""
    ws, hs = oracle.orb_level_dims(w, h, nlevels)
    out = []
    for lw, lh in zip(ws.tolist(), hs.tolist()):
        vw, vh = lw - 38, lh - 38
        ncx, ncy = (vw + 31) // 32 if vw > 0 else 0, (vh + 31) // 32 if vh > 0 else 0
        out.append((ncx, ncy) if ncx and ncy else (0, 0))
    return out


def _plan(ctx, w, h, batch, K=1000, nlevels=8, ini_th=20, min_th=7):
    from gslam_amd.orb import OrbExtractor
    return OrbExtractor(ctx, w, h, max_batch=batch, n_features=K, n_levels=nlevels, ini_th=ini_th, min_th=min_th)


def _extract(ex, frames, pad=0, counters=False):
    """One gh_orb_extract_dev call on `frames` laid out with row stride w + pad (the pad bytes hold noise that no
    result may depend on).  -> ((kps B x K x 7 f32, desc B x K x 32, counts), debug counters or None)"""
    import torch
    B, h, w = frames.shape
    buf = np.random.default_rng(B * w + pad).integers(0, 256, (B, h, w + pad), dtype=np.uint8)
    buf[:, :, :w] = frames
    if counters:
        ex.debug_counters(enable=True, read=False)
    kps, desc, counts = ex.extract(torch.from_numpy(buf).cuda())
    torch.cuda.synchronize()
    out = kps.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()
    return out, (ex.debug_counters(enable=False) if counters else None)


def _gpu(ctx, frames, K=1000, nlevels=8, ini_th=20, min_th=7, pad=0, counters=False):
    B, h, w = frames.shape
    ex = _plan(ctx, w, h, B, K, nlevels, ini_th, min_th)
    try:
        return _extract(ex, frames, pad, counters)
    finally:
        ex.close()


def _oracle(oracle, frames, K=1000, nlevels=8, ini_th=20, min_th=7):
    ek, ed, ec = oracle.orb_extract_batch(frames, K, nlevels=nlevels, ini_th=ini_th, min_th=min_th, threads=THREADS)
    return ek.view(np.uint8).reshape(len(ec), K, 28), ed, ec


def _same(got, exp, what):
    """got: the GPU's (kps, desc, counts); exp: the oracle's (or another GPU call's) for the same frames.  All 28 + 32
    bytes of every record, the counts and the zero tail; the first differing frame / record is named."""
    gk, gd, gc = got
    B, K = gc.shape[0], gk.shape[1]
    gk = np.ascontiguousarray(gk).view(np.uint8).reshape(B, K, 28)
    ek, ed, ec = exp
    ek = np.ascontiguousarray(ek).view(np.uint8).reshape(B, K, 28)
    assert ec.shape[0] == B, what
    bad = np.nonzero(gc != ec)[0]
    assert len(bad) == 0, f"{what}: frame {bad[0]}: count {gc[bad[0]]} vs {ec[bad[0]]} ({len(bad)} frames differ)"
    live = np.arange(K)[None, :] < gc[:, None]
    tail = ~live & ((gk != 0).any(-1) | (gd != 0).any(-1))
    if tail.any():
        f, i = np.argwhere(tail)[0]
        raise AssertionError(f"{what}: frame {f}: record {i} past the count {gc[f]} is not zero")
    diff = (gk != ek).any(-1) | (gd != ed).any(-1)
    if diff.any():
        f, i = np.argwhere(diff)[0]
        kd = np.nonzero(gk[f, i] != ek[f, i])[0]
        raise AssertionError(f"{what}: frame {f} of {B}: record {i} of {gc[f]} differs ({int(diff.sum())} records in "
                             f"{len(np.unique(np.argwhere(diff)[:, 0]))} frames); keypoint bytes {kd.tolist()}, "
                             f"descriptor bytes {np.nonzero(gd[f, i] != ed[f, i])[0].tolist()}; "
                             f"got {gk[f, i].view(np.float32)[:5]}, expected {ek[f, i].view(np.float32)[:5]}")


def _prefix(res, n):
    return tuple(a[:n] for a in res)


# ---------------------------------------------------------------- A. threshold twins
@pytest.mark.parametrize("w,h,batches,sides", [
    (640, 480, (13, 14, 55), ("small", "per_level", "overlap")),
    (1241, 376, (8, 9, 36), ("small", "per_level", "overlap")),    # stride 1241: level 0 staged (copy_rows_kernel)
    (1024, 512, (8, 9), ("small", "per_level")),                   # 8 frames are exactly 4 << 20 pixels: still small
], ids=["640x480", "1241x376", "1024x512"])
def test_threshold_twins(ctx, oracle, w, h, batches, sides):
    """The same frames on both sides of each dispatch threshold: the shared frames bit-identical across the calls, every
    frame equal to the oracle."""
    for n, side in zip(batches, sides):
        assert side == ("overlap" if overlap(n, w, h) else "per_level" if per_level(n, w, h) else "small"), (n, side)
    frames = _frames(w, h, max(batches), seed=11 + w)
    big, _ = _gpu(ctx, frames)
    _same(big, _oracle(oracle, frames), f"{max(batches)} x {w}x{h}")
    for n in batches[:-1]:
        small, _ = _gpu(ctx, frames[:n])
        _same(small, _prefix(big, n), f"{n} x {w}x{h} against the first {n} frames of the {max(batches)}-frame call")


# ---------------------------------------------------------------- B. geometry sweep
@pytest.mark.parametrize("w,h,pad", [(1023, 577, 1), (517, 389, 3), (2047, 129, 61), (131, 1029, 16), (333, 257, 0),
                                     (1241, 376, 16)])
def test_geometry_sweep(ctx, oracle, w, h, pad):
    """The first batch above 4 << 20 pixels of each geometry: odd ncx / ncy, levels with nby <= 2 or nbx == 1 (no tile
    takes the MFMA resize), level 7 without cells (2047x129, 131x1029), aligned (1023 + 1) and staged strides.  Every
    pyramid level >= 1 of the first and the last frame against the oracle's, to locate a fused-resize fault."""
    B = first_per_level(w, h)
    assert per_level(B, w, h) and not per_level(B - 1, w, h) and not overlap(B, w, h)
    grid = _grid(oracle, w, h)
    fast = [g for g in grid if g[0]]
    assert any(ncx % 2 or ncy % 2 for ncx, ncy in fast)
    assert any((ncy + 1) // 2 <= 2 or (ncx + 1) // 2 == 1 for ncx, ncy in fast)
    if (w, h) in ((2047, 129), (131, 1029)):
        assert grid[7] == (0, 0) and grid[6] != (0, 0)
    frames = _frames(w, h, B, offset=w % 15, seed=w * h)
    ex = _plan(ctx, w, h, B)
    try:
        got, _ = _extract(ex, frames, pad)
        for f in (0, B - 1):
            for l in range(1, 8):
                assert np.array_equal(ex.debug_level(f, l), oracle.orb_pyramid_level(frames[f], l)), \
                    f"{B} x {w}x{h} (stride {w + pad}): pyramid level {l} of frame {f}"
    finally:
        ex.close()
    _same(got, _oracle(oracle, frames), f"{B} x {w}x{h} (stride {w + pad})")


# ---------------------------------------------------------------- C. parameters
PARAMS = [dict(K=1), dict(K=7), dict(K=33), dict(K=20000),
          dict(nlevels=1), dict(nlevels=3), dict(nlevels=5), dict(nlevels=8),
          dict(ini_th=20, min_th=7), dict(ini_th=254, min_th=1), dict(ini_th=7, min_th=7), dict(ini_th=100, min_th=50),
          dict(ini_th=254, min_th=254), dict(ini_th=9, min_th=8)]


@pytest.mark.parametrize("i", range(len(PARAMS)), ids=["-".join(f"{k}{v}" for k, v in p.items()) for p in PARAMS])
def test_parameters(ctx, oracle, i):
    """14 x 640x480 (per-level, no overlap) mixed classes at the quota extremes, 1 .. 8 levels and the threshold
    corners.  K = 1 leaves levels 0 .. 6 with quota 0 and K = 7 levels 6 and 7: each such level gets the stand-alone
    resize of its successor inside the per-level loop."""
    prm = dict(K=1000, nlevels=8, ini_th=20, min_th=7)
    prm.update(PARAMS[i])
    B, w, h = 14, 640, 480
    assert per_level(B, w, h) and not overlap(B, w, h)
    if prm["K"] == 1:
        assert oracle.orb_quotas(1).tolist() == [0] * 7 + [1]
    frames = _frames(w, h, B, offset=i, seed=300 + 31 * i)
    got, _ = _gpu(ctx, frames, **prm)
    _same(got, _oracle(oracle, frames, **prm), f"{B} x {w}x{h} {prm}")


@pytest.mark.parametrize("w,h,K", [(640, 480, 1), (640, 480, 7), (131, 1029, 1000)])
def test_levels_without_fast_pass_under_overlap(ctx, oracle, w, h, K):
    """With the select overlap, a level without a FAST pass (quota 0, or no cells: level 7 of 131x1029) still gets its
    own select launch on the side stream (its level_cnt = 0) and its successor's stand-alone resize."""
    B = OVERLAP_MIN_PX // (w * h) + 1
    assert overlap(B, w, h) and not overlap(B - 1, w, h)
    assert 0 in oracle.orb_quotas(K).tolist() or _grid(oracle, w, h)[7] == (0, 0)
    frames = _frames(w, h, B, offset=K % 15, seed=900 + K)
    got, _ = _gpu(ctx, frames, K=K)
    _same(got, _oracle(oracle, frames, K=K), f"{B} x {w}x{h} K={K}")


# ---------------------------------------------------------------- D. large levels
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("K", [8000, 20000])
def test_large_levels_streamed_select(ctx, oracle, B, K):
    """2560x1440: level 0 has 3476 cells (> 2048: the streaming select_kernel<false>) on saturated noise and a tie lattice;
    2 frames per-level, 5 frames per-level with the select overlap."""
    w, h = 2560, 1440
    assert per_level(B, w, h) and overlap(B, w, h) == (B == 5)
    ncx, ncy = _grid(oracle, w, h)[0]
    assert ncx * ncy > SEL_CACHED_CELLS
    frames = np.stack([CLASSES["noise" if f % 2 == 0 else "dots8"](w, h, 5 + f) for f in range(B)])
    got, _ = _gpu(ctx, frames, K=K)
    _same(got, _oracle(oracle, frames, K=K), f"{B} x {w}x{h} K={K}")


# ---------------------------------------------------------------- E. path switching on one plan
def test_path_switching_on_one_plan(ctx, oracle):
    """One plan, calls that alternate between the overlap, small and per-level paths, new content every call: no state
    that one path leaves in the plan may leak into the next call."""
    w, h = 640, 480
    seq = [55, 1, 14, 13, 55]
    assert [overlap(n, w, h) for n in seq] == [True, False, False, False, True]
    assert [per_level(n, w, h) for n in seq] == [True, False, True, False, True]
    ex = _plan(ctx, w, h, 55)
    try:
        for c, n in enumerate(seq):
            frames = _frames(w, h, n, offset=3 * c, seed=5000 + 1000 * c)
            got, _ = _extract(ex, frames)
            _same(got, _oracle(oracle, frames), f"call {c}: {n} x {w}x{h}")
    finally:
        ex.close()


# ---------------------------------------------------------------- F. fuzz
@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture, HealthCheck.data_too_large])
@given(w=st.integers(96, 720), h=st.integers(80, 540), pad=st.sampled_from([0, 1, 3, 16, 61]),
       K=st.one_of(st.integers(1, 40), st.integers(41, 4000)), nlevels=st.integers(1, 8),
       min_th=st.one_of(st.integers(1, 12), st.integers(13, 254)), ini_extra=st.one_of(st.just(0), st.integers(1, 60)),
       offset=st.integers(0, len(NAMES) - 1), seed=st.integers(0, 2 ** 31 - 1), extra=st.integers(0, 3))
def test_fuzz_per_level(ctx, oracle, w, h, pad, K, nlevels, min_th, ini_extra, offset, seed, extra):
    ini_th = min(254, min_th + ini_extra)
    B = first_per_level(w, h) + extra
    assert per_level(B, w, h)
    frames = _frames(w, h, B, offset=offset, seed=seed)
    prm = dict(K=K, nlevels=nlevels, ini_th=ini_th, min_th=min_th)
    got, _ = _gpu(ctx, frames, pad=pad, **prm)
    _same(got, _oracle(oracle, frames, **prm), f"{B} x {w}x{h} (stride {w + pad}) {prm}")


# ---------------------------------------------------------------- G. branch census
def test_branch_census_per_level(ctx, oracle):
    """The only case with the debug counters on: per-level calls must reach the branches test_branch_census asserts on
    the small path, plus the streaming select.  resize_passes counts the fused resize alone, so it is > 0 on every
    per-level call and 0 on its small twin (the first frames of the same batch, which must give the same records)."""
    runs = {  # name: (frames, K, small twin's batch)
        "mixed": (np.stack([CLASSES[n](640, 480, 3 + f) for f, n in
                            enumerate(["noise", "dots8", "checker2", "few_corners", "binary_noise", "mixed", "noise"] * 2)]),
                  1000, 13),
        "noise/K=20000": (np.stack([CLASSES["noise"](640, 480, 40 + f) for f in range(14)]), 20000, 13),
        "noise/2560x1440": (np.stack([CLASSES["noise"](2560, 1440, 60 + f) for f in range(2)]), 8000, 1),
    }
    dbg = {}
    for name, (frames, K, n_small) in runs.items():
        B, h, w = frames.shape
        assert per_level(B, w, h) and not per_level(n_small, w, h)
        got, d = _gpu(ctx, frames, K=K, counters=True)
        _same(got, _oracle(oracle, frames, K=K), f"{name} (counters on)")
        assert d["resize_passes"] > 0, (name, d)
        twin, ds = _gpu(ctx, frames[:n_small], K=K, counters=True)
        _same(twin, _prefix(got, n_small), f"{name}: the {n_small}-frame small twin")
        assert ds["resize_passes"] == 0, (name, ds)
        dbg[name] = d
    m = dbg["mixed"]
    assert m["cells"] > 0 and m["dense_cells"] > 0 and m["max_nz"] > 256, m
    assert m["overflow_cells"] > 0 and m["cap_cells"] > 0 and m["rank_dropped"] > 0, m
    assert m["sel_cut"] > 0 and m["sel_tie_split"] > 0, m
    assert m["starved_levels"] > 0 and m["unused_slots"] > 0, m
    assert m["sel_streamed"] == 0, m
    assert dbg["noise/K=20000"]["sel_overflow_cells"] > 0, dbg["noise/K=20000"]
    assert dbg["noise/2560x1440"]["sel_streamed"] > 0, dbg["noise/2560x1440"]


# ---------------------------------------------------------------- H. modes
@pytest.mark.parametrize("mode", ["steering", "quadtree"])
def test_modes_at_overlap_size(ctx, oracle, mode):
    """55 x 640x480 mixed classes (an overlap-sized call) with continuous steering (the per-level path with the select
    overlap, then describe_kernel) / ORB-SLAM's quadtree distribution (enqueue_quadtree, which
    runs at every call size and never overlaps select)."""
    B, w, h = 55, 640, 480
    assert overlap(B, w, h)
    frames = _frames(w, h, B, offset=7, seed=777 if mode == "steering" else 888)
    ex = _plan(ctx, w, h, B)
    try:
        (ex.set_steering if mode == "steering" else ex.set_distribution)(1)
        got, _ = _extract(ex, frames)
    finally:
        ex.close()
    (oracle.orb_set_steer if mode == "steering" else oracle.orb_set_distribution)(1)
    try:
        exp = _oracle(oracle, frames)
    finally:
        oracle.orb_set_steer(0)
        oracle.orb_set_distribution(0)
    _same(got, exp, f"{B} x {w}x{h} {mode}")


# ---------------------------------------------------------------- I. the default plan
def test_default_plan_gives_the_oracle_bytes(ctx, oracle):
    """One per-level batch through a plan with default parameters, against the oracle."""
    B, w, h = 14, 640, 480
    assert per_level(B, w, h)
    frames = _frames(w, h, B, offset=5, seed=4242)
    got, _ = _gpu(ctx, frames)
    _same(got, _oracle(oracle, frames), f"{B} x {w}x{h} default plan")
