"""The workspace layout of the dense solve (gslam_amd/csrc/dense_solve.h: one function sizes and places dinv, work, xwork, xh, the
single-launch state and info for chol.hip, ba.hip and chol_cr.hip) checked on the CPU under AddressSanitizer + UBSan: builds
tools/dense_layout_check.cpp with g++ (the layout is host-only C++ once __HIP_PLATFORM_AMD__ is defined) and runs its sweep over
n, extra_rows and the CU count.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_layout_segments_sizes_and_xwork_reach(tmp_path):
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "dense_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gslam_amd", "csrc"), "-I/opt/rocm/include",
           os.path.join(ROOT, "tools", "dense_layout_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "150 layouts checked, 0 failures" in r.stdout, r.stdout[-3000:]
