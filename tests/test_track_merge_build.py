"""Build check (no GPU) of the kernels behind gh_merge_points_dev (gslam_amd/csrc/track_merge.hip), read from the code objects of
the shipped library as tests/test_build_resources.py reads them: they are in the library under their common prefix, and none
of them touches scratch memory, spills a register or needs more than 64 vector registers."""
import os
import re

import pytest

from test_build_float_mode import LIB, LLVM
from test_build_resources import _kernels

EXPECTED = ("mrg_init_kernel", "mrg_union_kernel", "mrg_label_kernel", "mrg_key_kernel", "mrg_runs_kernel", "mrg_points_kernel",
            "mrg_emit_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm llvm-readelf")
def test_merge_kernels_are_in_the_library_and_use_no_scratch():
    assert os.path.exists(LIB), "build the library first (make lib)"
    rows = {n: r for n, r in _kernels().items() if re.search(r"\d+mrg_\w+_kernel", n)}
    assert len(rows) >= len(EXPECTED), sorted(rows)
    for frag in EXPECTED:
        assert any(re.search(r"\d+%s([A-Z]|$)" % frag, n) for n in rows), "kernel %s not found in the library" % frag
    for n, r in rows.items():
        assert int(r["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch" % (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0, "%s spills vector registers" % n
        # one lane per entry, a handful of live values: every one of them fits eight waves per SIMD
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 64, (n, r)
        print(n, r["vgpr_count"], r.get("sgpr_count"), r.get("group_segment_fixed_size"))
