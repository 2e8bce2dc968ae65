"""Build check (no GPU) of the kernels behind gh_describe_points_dev (gslam_amd/csrc/point_describe.hip), read from the code
objects of the shipped library as tests/test_build_resources.py reads them: they are in the library under their common prefix,
none of them touches scratch memory or spills a register, each fits four waves per SIMD (VGPR + AGPR <= 128: the wide kernel
holds a descriptor and little else) and 64 KB of LDS per workgroup."""
import os
import re

import pytest

from test_build_float_mode import LIB, LLVM
from test_build_resources import _kernels

EXPECTED = ("pdsc_keys_kernel", "pdsc_narrow_kernel", "pdsc_wide_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm llvm-readelf")
def test_describe_kernels_are_in_the_library_and_use_no_scratch():
    assert os.path.exists(LIB), "build the library first (make lib)"
    rows = {n: r for n, r in _kernels().items() if re.search(r"\d+pdsc_\w+_kernel", n)}
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
