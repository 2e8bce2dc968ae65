"""gslam_amd/devargs.py without a build and without a GPU: the argument check raises with the argument's name (also under
python -O), the three pointer rules give NULL / 0 / the dummy address where the C contract wants them, and alloc keeps the order
of its table.  A cuda tensor cannot exist here, so a valid argument is not among the cases: the GPU suites of the wrappers cover
it with every call they make."""
import os
import subprocess
import sys

import pytest
import torch

from gslam_amd import devargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Cuda:
    """A tensor that says it is on the device: every other answer is the CPU tensor's own."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_dev_names_the_argument_it_rejects():
    with pytest.raises(ValueError, match=r"^idx1: .*cuda"):
        devargs.dev("idx1", torch.zeros(4, dtype=torch.int32), "int32")
    with pytest.raises(ValueError, match=r"^idx1: .*float32"):
        devargs.dev("idx1", _Cuda(torch.zeros(4, dtype=torch.float32)), "int32")
    with pytest.raises(ValueError, match=r"^kps: .*contiguous"):
        devargs.dev("kps", _Cuda(torch.zeros((4, 8), dtype=torch.float32)[:, ::2]), "float32")
    with pytest.raises(ValueError, match=r"^counts: .*4 elements.*expected 3"):
        devargs.dev("counts", _Cuda(torch.zeros(4, dtype=torch.int32)), "int32", 3)
    with pytest.raises(ValueError, match=r"^cam_pose: .*multiple of 7"):
        devargs.dev("cam_pose", _Cuda(torch.zeros(8, dtype=torch.float64)), "float64", multiple_of=7)
    with pytest.raises(ValueError, match=r"^node_point: .*None"):
        devargs.dev("node_point", None, "int32")


def test_dev_passes_what_is_valid_and_an_optional_none():
    t = _Cuda(torch.zeros((2, 7), dtype=torch.float64))
    assert devargs.dev("cam_pose", t, "float64", 14, multiple_of=7) is t
    assert devargs.dev("keep", None, "uint8", 5, optional=True) is None
    with pytest.raises(ValueError, match=r"^keep: "):  # optional lets None through, nothing else
        devargs.dev("keep", torch.zeros(5, dtype=torch.uint8), "uint8", 5, optional=True)


def test_dev_raises_under_python_O():
    code = ("import sys, torch\n"
            "assert False, 'asserts must be off in this interpreter'\n"
            "sys.path.insert(0, %r)\n"
            "from gslam_amd import devargs\n"
            "try:\n"
            "    devargs.dev('idx1', torch.zeros(4, dtype=torch.float32), 'int32')\n"
            "except ValueError as e:\n"
            "    print('raised', e)\n" % ROOT)
    r = subprocess.run([sys.executable, "-O", "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("raised idx1: "), r.stdout


def test_pointer_rules():
    empty, full = torch.zeros(0, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    assert devargs.ptr(None) is None
    assert devargs.ptr(empty).value in (None, 0)
    assert devargs.ptr(full).value == full.data_ptr() != 0
    assert devargs.ptr_array(empty).value == 256
    assert devargs.ptr_array(full).value == full.data_ptr()
    with pytest.raises(ValueError):
        devargs.ptr_array(None)
    assert devargs.ptr_opt(None) is None
    assert devargs.ptr_opt(empty).value == 256
    assert devargs.ptr_opt(full).value == full.data_ptr()


def test_alloc_keeps_the_order_shapes_and_dtypes_of_its_table():
    kept = torch.ones(2, dtype=torch.int32)
    spec = {"b": ((3, 2), "float64"), "a": (5, "uint8", True), "skipped": None, "c": ((0, 7), "int32"),
            "in_place": kept, "z": ((4, 4), "float64", True)}
    out = devargs.alloc("cpu", spec)
    assert list(out) == list(spec)
    assert [(tuple(out[k].shape), out[k].dtype) for k in ("b", "a", "c", "z")] == [
        ((3, 2), torch.float64), ((5,), torch.uint8), ((0, 7), torch.int32), ((4, 4), torch.float64)]
    assert not out["a"].any() and not out["z"].any()
    assert out["skipped"] is None and out["in_place"] is kept
    assert all(out[k].is_contiguous() for k in ("b", "a", "c", "z"))


def test_recurring_groups():
    kps = _Cuda(torch.zeros((3, 8, 7), dtype=torch.float32))
    assert devargs.keypoints(kps) == (3, 8)
    with pytest.raises(ValueError, match=r"^kps: .*F x cap x 7"):
        devargs.keypoints(_Cuda(torch.zeros((3, 8, 6), dtype=torch.float32)))
    i32 = lambda *shape: _Cuda(torch.zeros(shape, dtype=torch.int32))
    assert devargs.pair_arrays(i32(3), 3, 8, i32(2), i32(2), i32(2, 8)) == 2
    assert devargs.pair_arrays(i32(3), 3, 8, i32(2), i32(2), i32(2, 8), _Cuda(torch.zeros((2, 8), dtype=torch.uint8)), "inlier") == 2
    with pytest.raises(ValueError, match=r"^counts: "):  # the check every entry makes: one count per frame
        devargs.pair_arrays(i32(4), 3, 8, i32(2), i32(2), i32(2, 8))
    with pytest.raises(ValueError, match=r"^pair_t: "):
        devargs.pair_arrays(i32(3), 3, 8, i32(2), i32(1), i32(2, 8))
    with pytest.raises(ValueError, match=r"^idx1: "):
        devargs.pair_arrays(i32(3), 3, 8, i32(2), i32(2), i32(2, 7))
    with pytest.raises(ValueError, match=r"^inlier: "):
        devargs.pair_arrays(i32(3), 3, 8, i32(2), i32(2), i32(2, 8), _Cuda(torch.zeros((2, 8), dtype=torch.int32)), "inlier")
    assert [c.value for c in devargs.pinhole((500, 501.5, 320, 240))] == [500.0, 501.5, 320.0, 240.0]

    import ctypes

    class S(ctypes.Structure):
        _fields_ = [("filled", ctypes.c_int)]

    given = S(7)
    assert devargs.defaults(given, S, None) is given
    made = devargs.defaults(None, S, lambda ref: setattr(ref._obj, "filled", 1))
    assert isinstance(made, S) and made.filled == 1
