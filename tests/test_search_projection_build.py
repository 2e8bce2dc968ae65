"""Build check (no GPU) of the kernels behind gh_search_projection_dev (gslam_amd/csrc/search_projection.hip), read from the code
objects of the shipped library as tests/test_build_resources.py reads them: they are in the library under their common prefix,
none of them touches scratch memory or spills a register, each fits four waves per SIMD (VGPR + AGPR <= 128) and 64 KB of LDS
per workgroup.  The host-only entries answer without a device: the defaults of the header, and the cell side that
tests/test_search_projection_cpu.py counts cells with."""
import ctypes as C
import os
import re

import pytest

from test_build_float_mode import LIB, LLVM
from test_build_resources import _kernels

EXPECTED = ("sproj_frames_kernel", "sproj_grid_kernel", "sproj_search_kernel", "sproj_resolve_kernel", "sproj_finish_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm llvm-readelf")
def test_search_kernels_are_in_the_library_and_use_no_scratch():
    assert os.path.exists(LIB), "build the library first (make lib)"
    rows = {n: r for n, r in _kernels().items() if re.search(r"\d+sproj_\w+_kernel", n)}
    assert len(rows) >= len(EXPECTED), sorted(rows)
    for frag in EXPECTED:
        assert any(re.search(r"\d+%s([A-Z]|$)" % frag, n) for n in rows), "kernel %s not found in the library" % frag
    for n, r in rows.items():
        print(n, "vgpr", r["vgpr_count"], "agpr", r.get("agpr_count", 0), "sgpr", r.get("sgpr_count"), "lds",
              r.get("group_segment_fixed_size"), "scratch", r["private_segment_fixed_size"])
        assert int(r["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch" % (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, "%s spills registers" % n
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 128, (n, r)
        assert int(r.get("group_segment_fixed_size", 0)) <= 64 * 1024, (n, r)


def test_host_entries():
    import search_projection_restate as sr
    import test_search_projection_cpu as cpu
    from gslam_amd import hip
    assert C.sizeof(hip.SearchParams) == 80
    p = hip.SearchParams()
    hip.lib.gh_search_default_params(C.byref(p))
    assert {k: getattr(p, k) for k, _ in hip.SearchParams._fields_} == sr.DEFAULTS
    assert hip.lib.gh_search_cell_pixels() == cpu.CELL
