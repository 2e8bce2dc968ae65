"""GPU parity of undistort_kernel (through the C ABI) with oracle/undist_oracle.c on the adversarial classes of
tests/undist_cases.py, and with the reference's recorded outputs (tests/golden/undist_adversarial.npz) where the reference
defines the pixel.  tests/test_undist_adversarial_oracle.py shows on the CPU that each class reaches what it names and that
the oracle equals the plain restatement and the reference there; here every output byte is equal, zero fill included,
through the host entry, the device entry with dense frames, and the device entry with padded frame strides, whose padding
keeps its bytes.  Refused calls and refused tables return GH_ERR_ARG before any launch.

No case reads or writes out of bounds: every table here satisfies the plan's contract (asserted by the CPU census),
buffers cover batch x stride bytes, and the tables built to be refused are only ever passed to gh_undist_plan_create."""
import ctypes as C
import os

import numpy as np
import pytest

import undist_cases as uc

pytestmark = pytest.mark.gpu

GH_OK, GH_ERR_ARG = 0, 1  # include/gslam_hip.h
DIRTY = 0xAB
GOLD = os.path.join(os.path.dirname(__file__), "golden", "undist_adversarial.npz")

_expected = {}


def expected(oracle, name, label, ch, fast):
    """The oracle's output for (class, image, mode), computed once and shared (read only)."""
    key = (name, label, ch, fast)
    if key not in _expected:
        c = uc.case(name)
        _expected[key] = oracle.undistort(dict(c["images"])[label][ch], c["tables"], fast=fast)[0]
    return _expected[key]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _strided(plan, imgs, ch, fast, in_pad, out_pad, n_out):
    """gh_undistort_dev on frames `in_pad` / `out_pad` bytes apart beyond their size -> (status, out batch x stride u8)"""
    import torch
    from gslam_amd import hip
    B, n_in = len(imgs), imgs[0].size
    src = np.full((B, n_in + in_pad), DIRTY, np.uint8)
    for b, im in enumerate(imgs):
        src[b, :n_in] = im.reshape(-1)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((B, n_out * ch + out_pad), DIRTY, dtype=torch.uint8, device="cuda")
    st = hip.lib.gh_undistort_dev(plan.h, _p(d_in), ch, B, C.c_size_t(n_in + in_pad), _p(d_out), C.c_size_t(n_out * ch + out_pad),
                                  1 if fast else 0)
    torch.cuda.synchronize()
    return st, d_out.cpu().numpy()


@pytest.mark.parametrize("name", list(uc.CASES))
def test_class_parity(ctx, oracle, name):
    import torch
    from gslam_amd.undist import Undistorter
    c = uc.case(name)
    t = c["tables"]
    n_out = t["w_out"] * t["h_out"]
    u = Undistorter(ctx, t)
    pixels = 0
    for label, imgs in c["images"]:
        for ch, fast in uc.MODES:
            want = expected(oracle, name, label, ch, fast)
            key = (name, label, ch, fast)
            got = u.undistort_host(imgs[ch], fast=fast)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (key, "host", int((got != want).sum()))
            dev = u.undistort(torch.from_numpy(imgs[ch][None]).cuda(), fast=fast)
            torch.cuda.synchronize()
            assert dev.cpu().numpy()[0].tobytes() == want.tobytes(), (key, "device")
            pixels += n_out
    # padded frame strides, batches of 1 and 3: frame b is the image rolled by b pixels
    label, imgs = c["images"][0]
    for ch, fast in uc.MODES:
        for B, in_pad, out_pad in ((1, 5, 3), (3, 37, 129)):
            frames = [np.roll(imgs[ch].reshape(-1, ch), b, axis=0).reshape(imgs[ch].shape) for b in range(B)]
            st, out = _strided(u, frames, ch, fast, in_pad, out_pad, n_out)
            assert st == GH_OK
            for b in range(B):
                want = expected(oracle, name, label, ch, fast) if b == 0 else oracle.undistort(frames[b], t, fast=fast)[0]
                assert out[b, :n_out * ch].tobytes() == want.tobytes(), (name, ch, fast, B, b)
            assert (out[:, n_out * ch:] == DIRTY).all(), (name, ch, fast, B, "padding written")
            pixels += B * n_out
    u.close()
    print(f"undistortion class {name}: {pixels} pixels compared over {len(uc.MODES)} modes")


@pytest.mark.parametrize("name", list(uc.REF_PAIRS))
def test_recorded_reference_parity(ctx, oracle, name):
    """Directly against the reference's recorded outputs where it defines the pixel, and the oracle on every byte."""
    from gslam_amd.undist import Undistorter
    g = np.load(GOLD)
    cam_in, cam_out = uc.REF_PAIRS[name]
    t = {k: g[f"{name}/{k}"] for k in ("remapX", "remapFast", "remapIdx", "remapCoef")}
    t.update(w_in=cam_in[0], h_in=cam_in[1], w_out=cam_out[0], h_out=cam_out[1])
    u = Undistorter(ctx, t)
    for ch, fast in uc.MODES:
        img = g[f"{name}/img{ch}"]
        got = u.undistort_host(img, fast=fast)
        eo, written = oracle.undistort(img, t, fast=fast)
        assert got.tobytes() == eo.tobytes(), (name, ch, fast)
        assert np.array_equal(written, g[f"{name}/written{ch}_{int(fast)}"].astype(bool))
        assert np.array_equal(got[written], g[f"{name}/out{ch}_{int(fast)}"][written]), (name, ch, fast)
        left_out = 1.0 - written.mean()
        print(f"reference pair {name} channels {ch} fast {int(fast)}: {written.size} pixels, {left_out:.4f} left out")
        assert left_out <= 0.10
    u.close()


def test_call_refusals_leave_the_plan_usable(ctx, oracle):
    import torch
    from gslam_amd import hip
    from gslam_amd.undist import Undistorter
    c = uc.case("origin")
    t, imgs = c["tables"], c["images"][0][1]
    n_in, n_out = t["w_in"] * t["h_in"], t["w_out"] * t["h_out"]
    u = Undistorter(ctx, t)
    d_in = torch.from_numpy(np.ascontiguousarray(imgs[4])).cuda()  # large enough for every channel count below
    d_out = torch.full((3 * n_out * 5,), DIRTY, dtype=torch.uint8, device="cuda")

    def call(ch, batch, in_stride, out_stride, fast, src=d_in, dst=d_out):
        return hip.lib.gh_undistort_dev(u.h, _p(src), ch, batch, C.c_size_t(in_stride), _p(dst), C.c_size_t(out_stride), fast)

    assert call(2, 1, n_in * 2, n_out * 2, 1) == GH_ERR_ARG and call(5, 1, n_in * 5, n_out * 5, 1) == GH_ERR_ARG
    assert call(0, 1, n_in, n_out, 1) == GH_ERR_ARG and call(2, 1, n_in * 2, n_out * 2, 0) == GH_ERR_ARG
    assert call(4, 1, n_in * 4, n_out * 4, 0) == GH_ERR_ARG                      # 4 channels bilinear
    assert call(1, 1, n_in - 1, n_out, 1) == GH_ERR_ARG and call(1, 1, n_in, n_out - 1, 1) == GH_ERR_ARG
    assert call(3, 1, n_in * 3 - 1, n_out * 3, 0) == GH_ERR_ARG and call(3, 1, n_in * 3, n_out * 3 - 1, 0) == GH_ERR_ARG
    assert call(1, 1, n_in, n_out, 1, src=None) == GH_ERR_ARG and call(1, 1, n_in, n_out, 1, dst=None) == GH_ERR_ARG
    assert call(1, 65536, n_in, n_out, 1) == GH_ERR_ARG and call(1, -1, n_in, n_out, 1) == GH_ERR_ARG
    assert hip.lib.gh_undistort_dev(None, _p(d_in), 1, 1, C.c_size_t(n_in), _p(d_out), C.c_size_t(n_out), 1) == GH_ERR_ARG
    host_out = np.full(n_out * 5, DIRTY, np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert hip.lib.gh_undistort_host(u.h, hp(imgs[4]), 2, hp(host_out), 1) == GH_ERR_ARG
    assert hip.lib.gh_undistort_host(u.h, hp(imgs[4]), 4, hp(host_out), 0) == GH_ERR_ARG
    assert hip.lib.gh_undistort_host(u.h, None, 1, hp(host_out), 1) == GH_ERR_ARG
    assert call(1, 0, n_in, n_out, 1) == GH_OK and call(3, 0, 0, 0, 0) == GH_OK   # batch = 0: nothing to do
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == DIRTY).all() and (host_out == DIRTY).all()      # nothing was launched
    for ch, fast in uc.MODES:                                                      # the plan still works
        assert u.undistort_host(imgs[ch], fast=fast).tobytes() == expected(oracle, "origin", "random", ch, fast).tobytes()
    u.close()


def _create_status(ctx, t, **over):
    """gh_undist_plan_create on a table dict with single arguments overridden -> status (a created plan is destroyed)."""
    from gslam_amd import hip
    a = dict(w_in=t["w_in"], h_in=t["h_in"], w_out=t["w_out"], h_out=t["h_out"],
             remapX=np.ascontiguousarray(t["remapX"], np.float32), remapFast=np.ascontiguousarray(t["remapFast"], np.int32),
             remapIdx=np.ascontiguousarray(t["remapIdx"], np.int32), remapCoef=np.ascontiguousarray(t["remapCoef"], np.float32))
    a.update(over)
    pv = lambda z: None if z is None else z.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    st = hip.lib.gh_undist_plan_create(ctx.h, a["w_in"], a["h_in"], a["w_out"], a["h_out"], pv(a["remapX"]), pv(a["remapFast"]),
                                       pv(a["remapIdx"]), pv(a["remapCoef"]), C.byref(h))
    if st == GH_OK:
        hip.lib.gh_undist_plan_destroy(h)
    else:
        assert not h.value
    return st


def test_plan_creation_refuses_tables_outside_the_contract(ctx, oracle):
    """Only gh_undist_plan_create sees these tables; no undistortion ever runs on them."""
    from gslam_amd.undist import Undistorter
    c = uc.case("last_row_col")
    t = c["tables"]
    n_in, n_out = t["w_in"] * t["h_in"], t["w_out"] * t["h_out"]
    assert _create_status(ctx, t) == GH_OK
    for key in ("w_in", "h_in", "w_out", "h_out"):
        for bad in (0, -1):
            assert _create_status(ctx, t, **{key: bad}) == GH_ERR_ARG, (key, bad)
    for key in ("remapX", "remapFast", "remapIdx", "remapCoef"):
        assert _create_status(ctx, t, **{key: None}) == GH_ERR_ARG, key
    valid = int(np.nonzero(t["remapX"] > 0)[0][0])
    for pixel in (0, valid, n_out - 1):
        for slot in range(4):
            idx = t["remapIdx"].copy()
            idx[pixel, slot] = -1
            assert _create_status(ctx, t, remapIdx=idx) == GH_ERR_ARG, (pixel, slot, "negative index")
            idx[pixel, slot] = n_in + t["w_in"] + 1
            assert _create_status(ctx, t, remapIdx=idx) == GH_ERR_ARG, (pixel, slot, "index past the step")
            idx[pixel, slot] = n_in + t["w_in"]
            assert _create_status(ctx, t, remapIdx=idx) == GH_OK, (pixel, slot, "the largest index the reference holds")
    for pixel in (0, valid, n_out - 1):
        fast = t["remapFast"].copy()
        fast[pixel] = n_in
        assert _create_status(ctx, t, remapFast=fast) == GH_ERR_ARG, (pixel, "remapFast == n_in")
        fast[pixel] = n_in - 1
        assert _create_status(ctx, t, remapFast=fast) == GH_OK
    # the fast table has to agree with remapX: a negative remapFast under remapX > 0 would send the 4-channel fast path
    # in front of the image
    for pixel in np.nonzero(t["remapX"] > 0)[0][[0, -1]]:
        for neg in (-1, -2, np.iinfo(np.int32).min):
            fast = t["remapFast"].copy()
            fast[pixel] = neg
            assert _create_status(ctx, t, remapFast=fast) == GH_ERR_ARG, (pixel, neg)
    bad = int(np.nonzero(t["remapX"] < 0)[0][0])
    x = t["remapX"].copy()
    for v in (np.float32(1e-45), np.float32(0.5), np.float32(np.inf)):
        x[bad] = v
        assert _create_status(ctx, t, remapX=x) == GH_ERR_ARG, v
    for v in (np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(-7)):  # not positive: nothing reads remapFast there
        x[bad] = v
        assert _create_status(ctx, t, remapX=x) == GH_OK, v
    # the context still makes working plans
    u = Undistorter(ctx, t)
    img = c["images"][0][1][4]
    assert u.undistort_host(img, fast=True).tobytes() == expected(oracle, "last_row_col", "random", 4, True).tobytes()
    u.close()
