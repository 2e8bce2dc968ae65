"""Build check (no GPU) of the kernels behind gh_ba_window_dev and gh_ba_window_scatter_dev (gslam_amd/csrc/ba_window.hip), read
from the code objects of the shipped library as tests/test_build_resources.py reads them: they are in the library under their
common prefix, and none of them touches scratch memory or spills a register."""
import os
import re

import pytest

from test_build_float_mode import LIB, LLVM
from test_build_resources import _kernels

EXPECTED = ("baw_count_kernel", "baw_seen_kernel", "baw_shared_kernel", "baw_local_kernel", "baw_points_kernel", "baw_fixed_kernel",
            "baw_flags_kernel", "baw_emit_kernel", "baw_scatter_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm llvm-readelf")
def test_window_kernels_are_in_the_library_and_use_no_scratch():
    assert os.path.exists(LIB), "build the library first (make lib)"
    rows = {n: r for n, r in _kernels().items() if re.search(r"\d+baw_\w+_kernel", n)}
    assert len(rows) >= 4, sorted(rows)
    for frag in EXPECTED:
        assert any(re.search(r"\d+%s([A-Z]|$)" % frag, n) for n in rows), "kernel %s not found in the library" % frag
    for n, r in rows.items():
        assert int(r["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch" % (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0, "%s spills vector registers" % n
        # one lane per entry, a handful of live values: every one of them fits eight waves per SIMD
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 64, (n, r)
        print(n, r["vgpr_count"], r.get("group_segment_fixed_size"))
