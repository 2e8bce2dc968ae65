"""Launch census of gh_orb_extract_dev: which kernels one call launches, and how often.

Every schedule of the ORB front end is bit-exact against the oracle, so a call that takes the wrong schedule passes every
parity test and only loses speed.  This file pins the launches: one extract call under the context's profiler
(ctx.prof_enable / prof_collect count launches per GH_LAUNCH label), compared with a restatement of the schedule rule
(gslam_amd/csrc/orb.hip, orb_schedule) written from the oracle's level geometry and quotas, never from the library:
  px = batch * w * h
  px <= 4 << 20   all-levels: L - 1 stand-alone resizes, ONE orb_fast_cells for every level, one select
  px >  4 << 20   per-level: one orb_fast_cells per level with cells and a quota (it builds the next level inside the
                  kernel); a level whose predecessor runs no FAST pass comes from the stand-alone resize; one select
  px >= 16 << 20  per-level with the select overlap: one select per level, the dead ones included
  distribution 1  quadtree: orb_fast_plane + orb_slam_cells per level whose cells fit the plane kernels, orb_slam_cells
                  from the image (and a stand-alone resize of the successor) where they do not, one orb_slam_quadtree
  level 0 is read in place when base, row stride and frame stride are multiples of 16, else staged by orb_copy_level0.
Profiling turns graph replay off (tests/test_orb_gpu.py holds the graph cache).  Where two kernels share a label -- cached
and streamed select, the three cell kernels, the two describes -- the sel_streamed counter and tests/orb_slam_mirror.py
stay the witnesses.
"""
import numpy as np
import pytest

import orb_slam_mirror as mirror
from test_orb_per_level_gpu import OVERLAP_MIN_PX, SMALL_MAX_PX, _grid, _plan

pytestmark = pytest.mark.gpu

L = 8
_BUFFERS = {}


def _buffer(batch, w, h, pad=0):
    """batch x h x (w + pad) bytes of noise on the GPU (the content decides no launch); cached, never written."""
    import torch
    key = (w, h, pad)
    if key not in _BUFFERS or _BUFFERS[key].shape[0] < batch:
        rng = np.random.default_rng(w * h + pad)
        _BUFFERS[key] = torch.from_numpy(rng.integers(0, 256, (batch, h, w + pad), dtype=np.uint8)).cuda()
    return _BUFFERS[key][:batch]


def _zero_copy(buf):
    """Level 0 is read from the caller's buffer: base, row stride and frame stride are multiples of 16."""
    return buf.data_ptr() % 16 == 0 and buf.stride(1) % 16 == 0 and buf.stride(0) % 16 == 0


def expected_default(oracle, batch, w, h, K, zero_copy):
    grid = _grid(oracle, w, h, L)
    quota = oracle.orb_quotas(K, L).tolist()
    fast = [ncx != 0 and q > 0 for (ncx, _), q in zip(grid, quota)]
    px = batch * w * h
    if px <= SMALL_MAX_PX:
        exp = {"orb_resize": L - 1, "orb_fast_cells": 1 if any(fast) else 0, "orb_select": 1}
    else:
        exp = {"orb_resize": sum(not fast[l - 1] for l in range(1, L)), "orb_fast_cells": sum(fast),
               "orb_select": L if px >= OVERLAP_MIN_PX else 1}
    exp["orb_describe"] = 1
    exp["orb_copy_level0"] = 0 if zero_copy else 1
    return {k: v for k, v in exp.items() if v}


def expected_quadtree(oracle, w, h, K, zero_copy):
    assert not mirror.refused(oracle, w, h, K, L)
    kern = [mirror.cell_kernel(oracle, lw, lh, q) for lw, lh, q in mirror.levels(oracle, w, h, K, L)]
    plane = [k in ("plane32", "plane40") for k in kern]
    exp = {"orb_fast_plane": sum(plane), "orb_slam_cells": sum(k is not None for k in kern), "orb_slam_quadtree": 1,
           "orb_resize": sum(not plane[l - 1] for l in range(1, L)), "orb_describe": 1,
           "orb_copy_level0": 0 if zero_copy else 1}
    return {k: v for k, v in exp.items() if v}


def census(ctx, ex, buf):
    """{label: launches} of one extract call."""
    import torch
    ctx.prof_enable(True)
    try:
        ex.extract(buf)
        torch.cuda.synchronize()
        prof = ctx.prof_collect()
    finally:
        ctx.prof_enable(False)
    return {k: v["launches"] for k, v in prof.items()}


def _one_call(ctx, oracle, batch, w, h, K=1000, pad=0, quadtree=False):
    buf = _buffer(batch, w, h, pad)
    ex = _plan(ctx, w, h, batch, K, L)
    try:
        if quadtree:
            ex.set_distribution(1)
        got = census(ctx, ex, buf)
    finally:
        ex.close()
    exp = expected_quadtree(oracle, w, h, K, _zero_copy(buf)) if quadtree else \
        expected_default(oracle, batch, w, h, K, _zero_copy(buf))
    assert got == exp, f"{batch} x {w}x{h} (stride {w + pad}), K = {K}"
    return got


def test_small_aligned(ctx, oracle):
    got = _one_call(ctx, oracle, 1, 320, 240, K=300)
    assert got == {"orb_resize": L - 1, "orb_fast_cells": 1, "orb_select": 1, "orb_describe": 1}


def test_small_staged_level0(ctx, oracle):
    got = _one_call(ctx, oracle, 1, 320, 240, K=300, pad=3)
    assert got == {"orb_copy_level0": 1, "orb_resize": L - 1, "orb_fast_cells": 1, "orb_select": 1, "orb_describe": 1}


def test_small_dead_levels(ctx, oracle):
    grid = _grid(oracle, 100, 77, L)
    assert grid[0] != (0, 0) and grid[-1] == (0, 0)
    got = _one_call(ctx, oracle, 1, 100, 77)
    assert got["orb_fast_cells"] == 1 and got["orb_resize"] == L - 1


def test_per_level(ctx, oracle):
    assert SMALL_MAX_PX < 5 * 1024 * 1024 < OVERLAP_MIN_PX
    assert all(g != (0, 0) for g in _grid(oracle, 1024, 1024, L)) and min(oracle.orb_quotas(1000, L)) > 0
    got = _one_call(ctx, oracle, 5, 1024, 1024)
    assert got == {"orb_fast_cells": L, "orb_select": 1, "orb_describe": 1}


def test_per_level_dead_levels(ctx, oracle):
    assert SMALL_MAX_PX < 545 * 100 * 77 < OVERLAP_MIN_PX
    dead = sum(g == (0, 0) for g in _grid(oracle, 100, 77, L))
    assert 0 < dead < L
    got = _one_call(ctx, oracle, 545, 100, 77)
    # the first dead level is still built inside its predecessor's FAST pass; every later one by the stand-alone resize
    assert got["orb_fast_cells"] == L - dead and got["orb_resize"] == dead - 1 and got["orb_select"] == 1


def test_per_level_zero_quotas(ctx, oracle):
    assert SMALL_MAX_PX < 14 * 640 * 480 < OVERLAP_MIN_PX
    assert oracle.orb_quotas(1, L).tolist() == [0] * 7 + [1]
    got = _one_call(ctx, oracle, 14, 640, 480, K=1)
    assert got == {"orb_resize": L - 1, "orb_fast_cells": 1, "orb_select": 1, "orb_describe": 1}


def test_overlap(ctx, oracle):
    assert 17 * 1024 * 1024 >= OVERLAP_MIN_PX
    got = _one_call(ctx, oracle, 17, 1024, 1024)
    assert got == {"orb_fast_cells": L, "orb_select": L, "orb_describe": 1}


def test_overlap_zero_quotas(ctx, oracle):
    assert 55 * 640 * 480 >= OVERLAP_MIN_PX
    got = _one_call(ctx, oracle, 55, 640, 480, K=1)
    assert got == {"orb_resize": L - 1, "orb_fast_cells": 1, "orb_select": L, "orb_describe": 1}


@pytest.mark.parametrize("batch,w,h", [(2, 640, 480), (1, 100, 77)], ids=["2x640x480", "1x100x77"])
def test_quadtree(ctx, oracle, batch, w, h):
    kern = [mirror.cell_kernel(oracle, lw, lh, q) for lw, lh, q in mirror.levels(oracle, w, h, 1000, L)]
    if (w, h) == (100, 77):  # level 0 has cells above 40 px (image kernel), the upper levels are dead
        assert kern[0] == "image" and kern[-1] is None
    else:
        assert all(k in ("plane32", "plane40") for k in kern)
    got = _one_call(ctx, oracle, batch, w, h, quadtree=True)
    assert "orb_select" not in got and got["orb_slam_quadtree"] == 1


def test_path_switching(ctx, oracle):
    """One plan, calls on both sides of both thresholds in turn: each call takes the schedule of its own size."""
    w, h, K = 640, 480, 1000
    buf = _buffer(55, w, h)
    ex = _plan(ctx, w, h, 55, K, L)
    try:
        for n, selects in ((55, L), (1, 1), (14, 1), (13, 1), (55, L)):
            got = census(ctx, ex, buf[:n])
            assert got == expected_default(oracle, n, w, h, K, _zero_copy(buf[:n])), f"{n} frames"
            assert got["orb_select"] == selects, f"{n} frames"
    finally:
        ex.close()
