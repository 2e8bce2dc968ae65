"""GPU parity of gh_two_view_batch_dev / gh_two_view_pairs_dev.  The batch is compared, byte for byte, with the scalar
restatement tests/two_view_restate.py on the census inputs of tests/two_view_cases.py (tests/test_two_view_cpu.py shows what
they reach); the pair entry is compared with the composition of the public pieces it promises to equal.  Output buffers go in
filled with 0xAB (7.0 for doubles)."""
import ctypes as C

import numpy as np
import pytest

import two_view_cases as tc
import two_view_restate as tv

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(**kw):
    from gslam_amd import estimator
    p = estimator.two_view_default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _run_batch(ctx, a, with_mask=True, nproblems=None):
    """gh_two_view_batch_dev on dirty output buffers -> dict of host arrays."""
    import torch
    from gslam_amd import hip
    n = len(a["offsets"]) - 1 if nproblems is None else nproblems
    rows = len(a["src"])
    E, src, dst, off = _dev(a["E"]), _dev(a["src"]), _dev(a["dst"]), _dev(a["offsets"][:n + 1])
    mask = _dev(a["mask"]) if with_mask else None
    out = dict(poses=torch.full((n, 7), tc.FILL_POINT, dtype=torch.float64, device="cuda"),
               points=torch.full((rows, 3), tc.FILL_POINT, dtype=torch.float64, device="cuda"),
               good=torch.full((rows,), tc.FILL_GOOD, dtype=torch.uint8, device="cuda"),
               counts=torch.full((n, 4), -5, dtype=torch.int32, device="cuda"),
               n_used=torch.full((n,), -5, dtype=torch.int32, device="cuda"),
               status=torch.full((n,), -5, dtype=torch.int32, device="cuda"))
    prm = _params(**tc.BATCH_PARAMS)
    st = hip.lib.gh_two_view_batch_dev(ctx.h, _ptr(E), a["e_stride"], _ptr(src), _ptr(dst), _ptr(off), n, _ptr(mask), C.byref(prm),
                                       *(_ptr(out[k]) for k in ("poses", "points", "good", "counts", "n_used", "status")))
    assert st == 0, (st, hip.lib.gh_last_error(ctx.h))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _expected_arrays(ex, nproblems=None, rows_end=None):
    n = len(ex["status"]) if nproblems is None else nproblems
    points = np.array(ex["points"], np.float64)
    good = np.array(ex["good"], np.uint8)
    if rows_end is not None:  # a prefix of the batch: later rows belong to nobody
        points[rows_end:], good[rows_end:] = tc.FILL_POINT, tc.FILL_GOOD
    return dict(poses=np.array(ex["poses"][:n], np.float64), points=points, good=good,
                counts=np.array(ex["counts"][:n], np.int32), n_used=np.array(ex["n_used"][:n], np.int32),
                status=np.array(ex["status"][:n], np.int32))


def _assert_same(got, want, names, offsets):
    for p, name in enumerate(names[:len(want["status"])]):  # per problem first: a failure names the case
        assert got["status"][p] == want["status"][p], (name, got["status"][p], want["status"][p], got["counts"][p], want["counts"][p])
        assert got["counts"][p].tolist() == want["counts"][p].tolist(), (name, got["counts"][p], want["counts"][p])
        assert got["n_used"][p] == want["n_used"][p], name
        assert got["poses"][p].tobytes() == want["poses"][p].tobytes(), (name, got["poses"][p], want["poses"][p])
        b, e = int(offsets[p]), int(offsets[p + 1])
        if 0 <= b < e <= len(want["good"]):
            assert np.array_equal(got["good"][b:e], want["good"][b:e]), (name, int(got["good"][b:e].sum()), int(want["good"][b:e].sum()))
            assert got["points"][b:e].tobytes() == want["points"][b:e].tobytes(), name
    for k in ("poses", "points", "good", "counts", "n_used", "status"):  # then everything, the rows nobody owns included
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("e_stride", (9, 12))
def test_batch_matches_the_restatement_bit_for_bit(ctx, e_stride):
    a = tc.batch_arrays(e_stride)
    got = _run_batch(ctx, a)
    _assert_same(got, _expected_arrays(tc.batch_expected()), a["names"], a["offsets"])
    assert (got["status"] == tv.OK).sum() >= 10 and got["good"][got["good"] != tc.FILL_GOOD].sum() > 1500


def test_batch_twice_and_without_a_mask(ctx):
    """The same batch run twice gives the same bytes; without a mask every row takes part (the problems in front of the
    first masked one, whose expected results are those of the masked run: their masks are all ones)."""
    a = tc.batch_arrays(12)
    one, two = _run_batch(ctx, a), _run_batch(ctx, a)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    n = a["names"].index("mask_holes")
    assert n > 15
    got = _run_batch(ctx, a, with_mask=False, nproblems=n)
    # (offsets[n] is the limit of this call: the rows behind it are not addressed)
    _assert_same(got, _expected_arrays(tc.batch_expected(), nproblems=n, rows_end=int(a["offsets"][n])), a["names"], a["offsets"])


def test_mirror_makes_the_same_call(ctx):
    import torch
    from gslam_amd import estimator
    a = tc.batch_arrays(12)
    n = len(a["offsets"]) - 1
    got = estimator.two_view_batch(ctx, _dev(a["E"]).view(n, 12), _dev(a["src"]), _dev(a["dst"]), _dev(a["offsets"]), _dev(a["mask"]),
                                   _params(**tc.BATCH_PARAMS))
    torch.cuda.synchronize()
    want = _expected_arrays(tc.batch_expected())
    limit = int(a["offsets"][-1])  # (the mirror hands out zeroed row buffers: rows nobody owns are zero there)
    for k, g in zip(("poses", "points", "good", "counts", "n_used", "status"), got):
        g = g.cpu().numpy()
        w = want[k]
        if k in ("points", "good"):
            owned = np.array(tc.batch_expected()["good"]) != tc.FILL_GOOD
            assert not g[~owned].any()
            g, w = g[owned], w[owned]
        assert g.tobytes() == w.tobytes(), k
    assert limit == len(a["src"])


def _pair_call(ctx, d, prm, npairs=None, cap=tc.CAP, thr=tc.PAIR_THR, fx=tc.FX, **null):
    """gh_two_view_pairs_dev on dirty buffers; `null`: names of arguments to pass as NULL."""
    import torch
    from gslam_amd import hip
    P = len(tc.PAIRS) if npairs is None else npairs
    Pa = len(tc.PAIRS)
    out = dict(models=torch.full((Pa, 12), 7.0, dtype=torch.float64, device="cuda"),
               inlier=torch.full((Pa, tc.CAP), 0xAB, dtype=torch.uint8, device="cuda"),
               n_corr=torch.full((Pa,), -5, dtype=torch.int32, device="cuda"),
               inliers=torch.full((Pa,), -5, dtype=torch.int32, device="cuda"),
               poses=torch.full((Pa, 7), 7.0, dtype=torch.float64, device="cuda"),
               points=torch.full((Pa, tc.CAP, 3), 7.0, dtype=torch.float64, device="cuda"),
               good=torch.full((Pa, tc.CAP), 0xAB, dtype=torch.uint8, device="cuda"),
               votes=torch.full((Pa, 4), -5, dtype=torch.int32, device="cuda"),
               status=torch.full((Pa,), -5, dtype=torch.int32, device="cuda"))
    arg = lambda k, t: None if null.get(k) else _ptr(t)
    st = hip.lib.gh_two_view_pairs_dev(ctx.h, arg("kps", d["kps"]), _ptr(d["counts"]), cap, _ptr(d["pq"]), _ptr(d["pt"]), P,
                                       arg("idx1", d["idx1"]), _ptr(d["keep"]), C.c_double(fx), C.c_double(tc.FY), C.c_double(tc.CX),
                                       C.c_double(tc.CY), C.c_double(thr), C.c_uint64(tc.PAIR_SEED),
                                       C.byref(prm) if prm is not None else None, *(arg(k, out[k]) for k in out))
    torch.cuda.synchronize()
    return st, {k: v.cpu().numpy() for k, v in out.items()}


def _pair_inputs(with_keep=True):
    kps, counts, idx1, keep = tc.pair_frames()
    pq, pt = (np.array([p[k] for p in tc.PAIRS], np.int32) for k in (0, 1))
    host = dict(kps=kps, counts=counts, idx1=idx1, keep=keep if with_keep else None, pq=pq, pt=pt)
    dev = dict(kps=_dev(kps.view(np.float32).reshape(3, tc.CAP, 7)), counts=_dev(counts), idx1=_dev(idx1),
               keep=_dev(keep) if with_keep else None, pq=_dev(pq), pt=_dev(pt))
    return host, dev


@pytest.mark.parametrize("with_keep", (True, False))
def test_pairs_equal_the_composition(ctx, with_keep):
    """gather + normalisation in numpy float64 + estimate_batch(ESSENTIAL) + two_view_batch, scattered back to query rows,
    against the one call: every output, byte for byte.  The true pair and its reverse come back OK with the generator's
    pose to 1e-6 (noise: the float32 rounding of the keypoint records only, see two_view_cases)."""
    import torch
    from gslam_amd import estimator, hip
    host, dev = _pair_inputs(with_keep)
    prm = _params()
    st, got = _pair_call(ctx, dev, prm)
    assert st == 0, hip.lib.gh_last_error(ctx.h)

    corr = estimator.correspondences_from_matches(host["kps"], host["counts"], host["pq"], host["pt"], host["idx1"], host["keep"])
    P = len(tc.PAIRS)
    src = np.concatenate([tc.normalise(s) for s, _, _ in corr])
    dst = np.concatenate([tc.normalise(d) for _, d, _ in corr])
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([len(r) for _, _, r in corr])
    d_src, d_dst, d_off = _dev(src), _dev(dst), _dev(off)
    models, mask, inliers = estimator.estimate_batch(ctx, estimator.ESSENTIAL, d_src, d_dst, d_off, tc.PAIR_THR, tc.PAIR_SEED)
    poses, points, good, counts, n_used, status = estimator.two_view_batch(ctx, models, d_src, d_dst, d_off, mask, prm)
    torch.cuda.synchronize()
    models, mask, inliers, poses, points, good, counts, n_used, status = (
        t.cpu().numpy() for t in (models, mask, inliers, poses, points, good, counts, n_used, status))
    want = dict(models=models, inlier=np.zeros((P, tc.CAP), np.uint8), n_corr=np.diff(off).astype(np.int32), inliers=inliers,
                poses=poses, points=np.zeros((P, tc.CAP, 3)), good=np.zeros((P, tc.CAP), np.uint8), votes=counts, status=status)
    for p, (_, _, rows) in enumerate(corr):
        want["inlier"][p, rows] = mask[off[p]:off[p + 1]]
        want["good"][p, rows] = good[off[p]:off[p + 1]]
        want["points"][p, rows] = points[off[p]:off[p + 1]]
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert n_used.tolist() == inliers.tolist()  # the two-view kernel ran on the inliers of the fit
    assert got["n_corr"].tolist()[2:] == [0, 0] and got["status"].tolist() == [tv.OK, tv.OK, tv.NO_MODEL, tv.NO_MODEL]
    truth = ((tc.R_PAIR, tc.T_PAIR), (tc.R_PAIR.T, -tc.R_PAIR.T @ tc.T_PAIR))
    for p in (0, 1):
        assert 150 < got["inliers"][p] < got["n_corr"][p] and got["good"][p].sum() >= 0.9 * got["inliers"][p]
        assert got["votes"][p].max() == got["good"][p].sum()
        Rg = np.array(tv.rotation_of(got["poses"][p, :4].tolist())).reshape(3, 3)
        R, t = truth[p]
        err = max(np.abs(Rg - R).max(), np.abs(got["poses"][p, 4:] - t / np.linalg.norm(t)).max())
        print("pair", tc.PAIRS[p], "pose error %.3e" % err)
        assert err <= 1e-6, err
        X = got["points"][p][got["good"][p] == 1]
        assert (X[:, 2] > 0).all()
    if with_keep:  # the mirror makes the same call
        m = estimator.two_view_pairs(ctx, dev["kps"], dev["counts"], dev["pq"], dev["pt"], dev["idx1"], dev["keep"],
                                     (tc.FX, tc.FY, tc.CX, tc.CY), tc.PAIR_THR, tc.PAIR_SEED)
        torch.cuda.synchronize()
        for k in want:
            assert m[k].cpu().numpy().tobytes() == want[k].tobytes(), k


def test_refusals(ctx):
    """Argument errors return GH_ERR_ARG without a launch: the dirty output buffers stay dirty."""
    import torch
    from gslam_amd import hip
    a = tc.batch_arrays(9)
    n = 4
    E, src, dst, off = _dev(a["E"]), _dev(a["src"]), _dev(a["dst"]), _dev(a["offsets"][:n + 1])
    outs = [torch.full(s, v, dtype=t, device="cuda") for s, v, t in (((n, 7), 7.0, torch.float64), ((len(a["src"]), 3), 7.0, torch.float64),
                                                                     ((len(a["src"]),), 0xAB, torch.uint8), ((n, 4), -5, torch.int32),
                                                                     ((n,), -5, torch.int32), ((n,), -5, torch.int32))]

    def call(ctxh=ctx.h, E=E, stride=9, src=src, dst=dst, off=off, n=n, prm=_params(), drop=None):
        o = [None if k == drop else _ptr(t) for k, t in enumerate(outs)]
        return hip.lib.gh_two_view_batch_dev(ctxh, _ptr(E), stride, _ptr(src), _ptr(dst), _ptr(off), n, None,
                                             C.byref(prm) if prm is not None else None, *o)

    bad = [dict(ctxh=None), dict(E=None), dict(src=None), dict(dst=None), dict(off=None), dict(n=-1), dict(stride=8), dict(stride=0),
           dict(prm=None), dict(prm=_params(min_parallax_cos=0.0)), dict(prm=_params(min_parallax_cos=1.0000001)),
           dict(prm=_params(min_parallax_cos=float("nan"))), dict(prm=_params(max_reproj=-1e-9)),
           dict(prm=_params(max_reproj=float("nan")))] + [dict(drop=k) for k in range(6)]
    for kw in bad:
        assert call(**kw) == GH_ERR_ARG, kw
    assert call(n=0) == 0 and call(n=0, E=None, src=None) == 0  # nothing to do is no error
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == v).all() for t, v in zip(outs, (7.0, 7.0, 0xAB, -5, -5, -5)))  # nothing was launched
    assert call(prm=_params(min_parallax_cos=1.0, max_reproj=0.0)) == 0  # the ends of the ranges are inside
    torch.cuda.synchronize()
    assert (outs[5].cpu().numpy() >= 0).all()

    # the pair entry
    _, dev = _pair_inputs()
    prm = _params()
    for kw in (dict(cap=65536), dict(cap=-1), dict(npairs=-1), dict(thr=-1.0), dict(thr=float("nan")), dict(fx=0.0), dict(fx=float("nan")),
               dict(kps=True), dict(idx1=True), dict(models=True), dict(points=True), dict(good=True), dict(votes=True),
               dict(status=True), dict(poses=True)):
        st, out = _pair_call(ctx, dev, prm, **kw)
        assert st == GH_ERR_ARG, kw
        assert (out["status"] == -5).all() and (out["good"] == 0xAB).all()
    assert _pair_call(ctx, dev, None)[0] == GH_ERR_ARG
    assert _pair_call(ctx, dev, _params(max_reproj=-1.0))[0] == GH_ERR_ARG
    assert _pair_call(ctx, dev, prm, npairs=0)[0] == 0
    st, out = _pair_call(ctx, dev, prm)  # the context is usable after a refusal
    assert st == 0 and out["status"].tolist() == [tv.OK, tv.OK, tv.NO_MODEL, tv.NO_MODEL]
