"""GPU parity of bf_match_band_pairs_kernel and match_mask_kernel (through the C ABI) with oracle/bf_oracle.c on the
adversarial classes of tests/band_mask_cases.py.  tests/test_band_mask_adversarial_oracle.py shows on the CPU that each
class reaches what it names and that the oracle equals the plain restatement there; here every one of the P x cap output
rows is equal bit for bit (idx1, d1, d2 of the rows < nq, -1 / 65535 / 65535 from nq to cap), the words behind P x cap keep
what they held, and refused calls return GH_ERR_ARG before any launch and leave buffers and context as they were.

No case reads or writes out of bounds: desc / kps / counts have the full F x cap extent, pair entries are frame numbers
below F, counts above cap are clamped by the kernel, the mask's back list covers every non-negative idx1 of its case."""
import ctypes as C

import numpy as np
import pytest

import band_mask_cases as bc

pytestmark = pytest.mark.gpu

GH_OK, GH_ERR_ARG = 0, 1  # include/gslam_hip.h
TAIL = 96
DIRTY_I32, DIRTY_U16, DIRTY_U8 = -5, 0xABAB, 0xAB

_expected = {}


def expected(oracle, name):
    """The oracle's outputs for a class, computed once and shared (read only)."""
    if name not in _expected:
        _expected[name] = bc.oracle_pairs(oracle, bc.band_case(name))
    return _expected[name]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _upload(case):
    import torch
    F, cap = case["desc"].shape[:2]
    kps = np.ascontiguousarray(case["kps"]).view(np.float32).reshape(F, cap, 7)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (case["desc"], kps, case["counts"], case["pair_q"], case["pair_t"])]


def _dirty(n):
    import torch
    return (torch.full((n + TAIL,), DIRTY_I32, dtype=torch.int32, device="cuda"),
            torch.full((n + TAIL,), DIRTY_U16 - 65536, dtype=torch.int16, device="cuda"),
            torch.full((n + TAIL,), DIRTY_U16 - 65536, dtype=torch.int16, device="cuda"))


def _download(out):
    import torch
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint16), out[2].cpu().numpy().view(np.uint16)


def _untouched(out, start=0):
    i, a, b = _download(out)
    return (i[start:] == DIRTY_I32).all() and (a[start:] == DIRTY_U16).all() and (b[start:] == DIRTY_U16).all()


def _band_call(ctx, dev, cap, npairs, bps, out, entry=None):
    from gslam_amd import hip
    desc, kps, counts, pq, pt = dev
    if entry is not None:
        return entry(ctx.h, _p(desc), _p(counts), cap, _p(pq), _p(pt), npairs, _p(out[0]), _p(out[1]), _p(out[2]))
    return hip.lib.gh_bf_match_band_pairs_dev(ctx.h, _p(desc), _p(kps), _p(counts), cap, _p(pq), _p(pt), npairs, C.c_float(bps),
                                              _p(out[0]), _p(out[1]), _p(out[2]))


def _same(got, want, n, key):
    for g, w, what in zip(got, want, ("idx1", "d1", "d2")):
        w = w.reshape(-1)
        assert g[:n].tobytes() == w.tobytes(), (key, what, int((g[:n] != w).sum()), np.nonzero(g[:n] != w)[0][:6].tolist())


@pytest.mark.parametrize("name", bc.BAND_NAMES)
def test_band_class_parity(ctx, oracle, name):
    case = bc.band_case(name)
    cap, P = case["desc"].shape[1], len(case["pair_q"])
    dev, out = _upload(case), _dirty(P * cap)
    assert _band_call(ctx, dev, cap, P, case["bps"], out) == GH_OK
    got = _download(out)
    want = expected(oracle, name)
    print(f"band class {name}: {P * cap} rows compared, {int((want[0] >= 0).sum())} with a match")
    _same(got, want, P * cap, name)
    assert _untouched(out, P * cap), (name, "tail written")
    for i, (j, a, b) in case["want"].items():  # and the hand-derived answers directly
        assert got[0][i] == j and got[1][i] == a and (b is None or got[2][i] == b), (name, i)


def test_wide_open_equals_the_plain_pair_matcher(ctx, oracle):
    from gslam_amd import hip
    case = bc.band_case("wide_open")
    cap, P = case["desc"].shape[1], len(case["pair_q"])
    dev, band, plain = _upload(case), _dirty(P * cap), _dirty(P * cap)
    assert _band_call(ctx, dev, cap, P, case["bps"], band) == GH_OK
    assert _band_call(ctx, dev, cap, P, None, plain, entry=hip.lib.gh_bf_match_pairs_popc_dev) == GH_OK
    for g, w in zip(_download(band), _download(plain)):
        assert g.tobytes() == w.tobytes()  # tail included


def test_band_refusals_and_empty_calls(ctx, oracle):
    case = bc.band_case("none_one_two")
    cap, P = case["desc"].shape[1], len(case["pair_q"])
    dev, out = _upload(case), _dirty(P * cap)
    bps = case["bps"]
    for what, kw in (("negative band", dict(bps=-1.0)), ("tiny negative band", dict(bps=-1e-30)), ("NaN band", dict(bps=float("nan"))),
                     ("cap above the index field", dict(cap=65536)), ("negative cap", dict(cap=-1)), ("negative pair count", dict(npairs=-1))):
        a = dict(cap=cap, npairs=P, bps=bps)
        a.update(kw)
        assert _band_call(ctx, dev, a["cap"], a["npairs"], a["bps"], out) == GH_ERR_ARG, what
        assert _untouched(out), what
    for k in range(5):  # a null input with work to do
        d = list(dev)
        d[k] = None
        assert _band_call(ctx, d, cap, P, bps, out) == GH_ERR_ARG, k
    for k in range(3):  # a null output
        o = list(out)
        o[k] = None
        assert _band_call(ctx, dev, cap, P, bps, o) == GH_ERR_ARG, k
    assert _untouched(out)
    # nothing to do: OK, nothing touched, null pointers are not looked at
    assert _band_call(ctx, dev, cap, 0, bps, out) == GH_OK and _band_call(ctx, dev, 0, P, bps, out) == GH_OK
    assert _band_call(ctx, [None] * 5, cap, 0, bps, [None] * 3) == GH_OK and _band_call(ctx, [None] * 5, 0, P, bps, [None] * 3) == GH_OK
    assert _untouched(out)
    # the context still works
    assert _band_call(ctx, dev, cap, P, bps, out) == GH_OK
    _same(_download(out), expected(oracle, "none_one_two"), P * cap, "after refusals")
    assert _untouched(out, P * cap)


# ---------------------------------------------------------------------------------------------------------- match mask
def _mask_call(ctx, c, keep, null_back=False):
    import torch
    from gslam_amd import hip
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    idx1, d1, d2 = up(c["idx1"]), up(c["d1"].view(np.int16)), up(c["d2"].view(np.int16))
    back = None if (c["back"] is None or null_back) else up(c["back"])
    st = hip.lib.gh_match_mask_dev(ctx.h, _p(idx1), _p(d1), _p(d2), len(c["idx1"]), _p(back), int(c["nt"]), int(c["max_dist"]),
                                   int(c["ratio_num"]), int(c["ratio_den"]), int(c["cross_check"]), _p(keep))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("name", list(bc.MASK_CLASSES))
def test_mask_class_parity(ctx, oracle, name):
    import torch
    rows = 0
    for nq in bc.MASK_NQ:
        for c in bc.mask_cases(name, nq):
            keep = torch.full((nq + TAIL,), DIRTY_U8, dtype=torch.uint8, device="cuda")
            assert _mask_call(ctx, c, keep) == GH_OK
            got = keep.cpu().numpy()
            want = oracle.match_mask(c["idx1"], c["d1"], c["d2"], c["back"], c["nt"], c["max_dist"], c["ratio_num"], c["ratio_den"],
                                     c["cross_check"])
            key = (name, nq, c["nt"], c["max_dist"], c["ratio_num"], c["ratio_den"])
            assert np.isin(got[:nq], (0, 1)).all(), key
            assert np.array_equal(got[:nq], want), (key, np.nonzero(got[:nq] != want)[0][:6].tolist())
            assert (got[nq:] == DIRTY_U8).all(), (key, "tail written")
            rows += nq
    print(f"mask class {name}: {rows} rows compared")


def test_mask_refusals_and_empty_calls(ctx, oracle):
    import torch
    from gslam_amd import hip
    nq = 257
    c = bc.mask_cases("cross", nq)[0]
    keep = torch.full((nq + TAIL,), DIRTY_U8, dtype=torch.uint8, device="cuda")
    assert _mask_call(ctx, c, keep, null_back=True) == GH_ERR_ARG            # cross-check without a back list
    assert _mask_call(ctx, dict(c, nt=-1), keep) == GH_ERR_ARG
    idx1 = torch.from_numpy(c["idx1"]).cuda()
    d = torch.from_numpy(c["d1"].view(np.int16)).cuda()
    back = torch.from_numpy(c["back"]).cuda()
    args = lambda i, a, b, n, k: hip.lib.gh_match_mask_dev(ctx.h, _p(i), _p(a), _p(b), n, _p(back), c["nt"], 256, 7, 10, 1, _p(k))
    assert args(idx1, d, d, -1, keep) == GH_ERR_ARG
    assert args(None, d, d, nq, keep) == GH_ERR_ARG and args(idx1, None, d, nq, keep) == GH_ERR_ARG
    assert args(idx1, d, None, nq, keep) == GH_ERR_ARG and args(idx1, d, d, nq, None) == GH_ERR_ARG
    assert args(None, None, None, 0, None) == GH_OK                        # nothing to do
    torch.cuda.synchronize()
    assert (keep.cpu().numpy() == DIRTY_U8).all()
    # a call without cross-check takes a null back list; the context still works
    off = bc.mask_cases("cross_off", nq)[0]
    assert off["back"] is None and _mask_call(ctx, off, keep) == GH_OK
    want = oracle.match_mask(off["idx1"], off["d1"], off["d2"], None, off["nt"], off["max_dist"], off["ratio_num"], off["ratio_den"], 0)
    got = keep.cpu().numpy()
    assert np.array_equal(got[:nq], want) and (got[nq:] == DIRTY_U8).all()
