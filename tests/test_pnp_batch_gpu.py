"""GPU tests of gh_pnp_refine_batch_dev / gh_pnp_batch_dev.  A problem that is optimised must equal, byte for byte, gh_ba_pnp
(ba.pnp) on its compacted rows; the start conversion and the classification are held to tests/pnp_restate.py; the chain is
held to the composition of the public calls; the oracle bounds are those of tests/ba_parity.py for the single call.  Output
buffers go in filled with 0xAB bytes, 7.0 doubles and -5 ints."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import pnp_batch_cases as pc
import pnp_restate as pr
from ba_parity import COST_RTOL, STATE_ATOL

pytestmark = pytest.mark.gpu

GH_ERR_ARG = 1  # include/gslam_hip.h
NO_START, TOO_FEW = 4, 5
OUT = ("poses", "info", "summaries", "inlier", "n_inliers")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _options(huber, max_iterations):
    from gslam_amd import ba
    return ba.default_options(huber_delta=huber, max_iterations=max_iterations)


def _dirty(nproblems, rows, info=True):
    import torch
    from gslam_amd import estimator
    return dict(poses=torch.full((nproblems, 7), pc.FILL_DOUBLE, dtype=torch.float64, device="cuda"),
                info=torch.full((nproblems, 36), pc.FILL_DOUBLE, dtype=torch.float64, device="cuda") if info else None,
                summaries=torch.full((nproblems, estimator.SUMMARY_DTYPE.itemsize), pc.FILL_BYTE, dtype=torch.uint8, device="cuda"),
                inlier=torch.full((rows,), pc.FILL_BYTE, dtype=torch.uint8, device="cuda"),
                n_inliers=torch.full((nproblems,), pc.FILL_INT, dtype=torch.int32, device="cuda"))


def _host(out):
    import torch
    from gslam_amd import estimator
    torch.cuda.synchronize()
    h = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
    h["summaries"] = h["summaries"].view(estimator.SUMMARY_DTYPE).reshape(h["summaries"].shape[:-1])
    return h


def _refine(ctx, X, m, offsets, starts, mask=None, nproblems=None, dof=63, huber=0.01, max_iterations=50, info=True, min_rows=0,
            threshold=pc.INLIER_THRESHOLD, nrows=None, allocated=None):
    """gh_pnp_refine_batch_dev on dirty output buffers (sized for `allocated` problems) -> dict of host arrays."""
    from gslam_amd import hip
    n = len(offsets) - 1 if nproblems is None else nproblems
    rows = len(X) if nrows is None else nrows
    out = _dirty(n if allocated is None else allocated, len(X), info)
    opt = _options(huber, max_iterations)
    dX, dm, doff, dstart = _dev(X), _dev(m), _dev(offsets[:n + 1]), _dev(starts)  # (held until the results are on the host)
    dmask = _dev(mask) if mask is not None else None
    st = hip.lib.gh_pnp_refine_batch_dev(ctx.h, _ptr(dX), _ptr(dm), _ptr(doff), n, rows, _ptr(dmask), _ptr(dstart),
                                         int(starts.shape[1]), dof, C.byref(opt), min_rows, C.c_double(threshold),
                                         *(_ptr(out[k]) for k in OUT))
    assert st == 0, (st, hip.lib.gh_last_error(ctx.h))
    return _host(out)


_census_runs = {}


def _census_run(ctx, oracle, name):
    """One call on the census batch per configuration, computed once and shared by the tests below."""
    if name not in _census_runs:
        b, cfg = pc.census(oracle), pc.CONFIGS[name]
        _census_runs[name] = _refine(ctx, b["X"], b["m"], b["offsets"], b["starts"], mask=b["mask"] if cfg["mask"] else None,
                                     dof=cfg["dof"], huber=cfg["huber"], max_iterations=cfg["max_iterations"], info=cfg["info"])
    return _census_runs[name]


def _same_as_single_call(ctx, got, p, X, m, start, dof, huber, max_iterations, info, name):
    """Problem p of `got` against ba.pnp on the rows X, m from `start`: bytes of pose, information, costs; equal counts."""
    from gslam_amd import ba
    pose, s, inf = ba.pnp(ctx, X, m, start, dof=dof, options=_options(huber, max_iterations), want_information=info)
    sm = got["summaries"][p]
    assert (sm["iterations"], sm["accepted"], sm["termination"]) == (s.iterations, s.accepted, s.termination), (name, sm, s.iterations, s.accepted, s.termination)
    assert sm["n_used"] == len(X), name
    assert got["poses"][p].tobytes() == pose.tobytes(), (name, got["poses"][p], pose)
    assert np.float64(sm["initial_cost"]).tobytes() == np.float64(s.initial_cost).tobytes(), (name, sm["initial_cost"], s.initial_cost)
    assert np.float64(sm["final_cost"]).tobytes() == np.float64(s.final_cost).tobytes(), (name, sm["final_cost"], s.final_cost)
    if info:
        assert got["info"][p].tobytes() == inf.tobytes(), name
    return s


@pytest.mark.parametrize("config", list(pc.CONFIGS))
def test_census_equals_the_single_call_bit_for_bit(ctx, oracle, config):
    b, cfg = pc.census(oracle), pc.CONFIGS[config]
    got = _census_run(ctx, oracle, config)
    used, moved = set(), 0
    for p, name in enumerate(b["names"]):
        lo, hi = int(b["offsets"][p]), int(b["offsets"][p + 1])
        rows = np.arange(lo, hi)
        if cfg["mask"]:
            rows = rows[b["mask"][lo:hi] != 0]
        used.add(len(rows))
        s = _same_as_single_call(ctx, got, p, b["X"][rows], b["m"][rows], b["starts"][p], cfg["dof"], cfg["huber"],
                                 cfg["max_iterations"], cfg["info"], name)
        moved += s.accepted > 0
        if cfg["dof"] == 0b111000:  # rotation only: translation bitwise the start's
            assert got["poses"][p][4:].tobytes() == b["starts"][p][4:].tobytes(), name
        if cfg["max_iterations"] == 0:
            assert got["poses"][p].tobytes() == b["starts"][p].tobytes() and got["summaries"][p]["iterations"] == 0, name
    assert {1, 3, 6, 255, 256, 257, 513} <= used
    assert cfg["max_iterations"] == 0 or 2 * moved >= len(b["names"])  # the census is optimised, not merely copied
    if not cfg["info"]:
        assert got["info"] is None


def test_a_prefix_leaves_the_later_problems_alone(ctx, oracle):
    b = pc.census(oracle)
    full = _census_run(ctx, oracle, "huber_se3_info_mask")
    P, k = len(b["names"]), 9
    got = _refine(ctx, b["X"], b["m"], b["offsets"], b["starts"], mask=b["mask"], nproblems=k, allocated=P)
    end = int(b["offsets"][k])
    for name in ("poses", "info", "n_inliers"):
        assert got[name][:k].tobytes() == full[name][:k].tobytes(), name
    assert got["summaries"][:k].tobytes() == full["summaries"][:k].tobytes()
    assert got["inlier"][:end].tobytes() == full["inlier"][:end].tobytes()
    assert (got["poses"][k:] == pc.FILL_DOUBLE).all() and (got["info"][k:] == pc.FILL_DOUBLE).all()
    assert (got["n_inliers"][k:] == pc.FILL_INT).all() and (got["inlier"][end:] == pc.FILL_BYTE).all()
    assert (got["summaries"][k:].view(np.uint8) == pc.FILL_BYTE).all()


@pytest.mark.parametrize("config", ["huber_se3_info_mask", "huber_rotation_info_nomask"])
def test_classification_equals_the_restatement(ctx, oracle, config):
    """inlier_dev at the device's own final pose, over ALL rows of every range, masked or not; rows nobody owns untouched."""
    b = pc.census(oracle)
    got = _census_run(ctx, oracle, config)
    for p, name in enumerate(b["names"]):
        lo, hi = int(b["offsets"][p]), int(b["offsets"][p + 1])
        want = pr.classify(got["poses"][p].tolist(), b["X"][lo:hi].tolist(), b["m"][lo:hi].tolist(), pc.INLIER_THRESHOLD)
        assert got["inlier"][lo:hi].tolist() == want, name
        assert got["n_inliers"][p] == sum(want), name
    assert (got["inlier"][int(b["offsets"][-1]):] == pc.FILL_BYTE).all()
    assert 0.5 * b["offsets"][-1] < got["n_inliers"].sum() < b["offsets"][-1]  # both answers occur


def test_negative_threshold_zero_fills(ctx, oracle):
    b = pc.census(oracle)
    k = 8
    got = _refine(ctx, b["X"], b["m"], b["offsets"], b["starts"], mask=b["mask"], nproblems=k, threshold=-1.0, allocated=k + 1)
    full = _census_run(ctx, oracle, "huber_se3_info_mask")
    end = int(b["offsets"][k])
    assert not got["inlier"][:end].any() and (got["inlier"][end:] == pc.FILL_BYTE).all()
    assert not got["n_inliers"][:k].any() and got["n_inliers"][k] == pc.FILL_INT
    assert got["poses"][:k].tobytes() == full["poses"][:k].tobytes()


def test_census_twice_gives_the_same_bytes(ctx, oracle):
    b, cfg = pc.census(oracle), pc.CONFIGS["huber_se3_info_mask"]
    one = _census_run(ctx, oracle, "huber_se3_info_mask")
    two = _refine(ctx, b["X"], b["m"], b["offsets"], b["starts"], mask=b["mask"])
    for k in OUT:
        assert one[k].tobytes() == two[k].tobytes(), k


def _degenerate(oracle):
    """Ranges and starts that are not regular, in one batch.  Valid ranges never overlap: the range that reaches past the
    arrays is followed by the reversed one that comes back."""
    cases = [pc.pnp_case(oracle, 300 + i, n, 0.002, 7) for i, n in enumerate((100, 150, 4, 80, 60, 70, 50, 40))]
    X = np.concatenate([c[0] for c in cases])
    m = np.concatenate([c[1] for c in cases])
    rows = len(X)
    b = np.cumsum([0] + [len(c[0]) for c in cases])
    names = ["regular", "empty", "zero_mask", "four_rows", "past_the_arrays", "reversed", "behind", "zero_start", "nan_start",
             "zero_quaternion", "inf_start"]
    #          regular      empty        zero_mask    four_rows    past           reversed          behind ...
    offsets = [b[0], b[1], b[1], b[2], b[3], b[3] + 1000, b[3], b[4], b[5], b[6], b[7], b[8]]
    src = [0, None, 1, 2, None, None, 3, 4, 5, 6, 7]  # the generated case behind each problem
    mask = np.ones(rows, np.uint8)
    mask[b[1]:b[2]] = 0
    starts = np.zeros((len(names), 7))
    for p, c in enumerate(src):
        starts[p] = cases[c][2] if c is not None else cases[0][2]
    q = starts[6, :4].copy()  # behind: the camera turned by pi about its own y axis, q <- q * (0, 1, 0, 0)
    starts[6, :4] = [q[3] * 0 + q[0] * 0 + q[1] * 0 - q[2] * 1, q[3] * 1 + q[1] * 0 + q[2] * 0 - q[0] * 0,
                     q[3] * 0 + q[2] * 0 + q[0] * 1 - q[1] * 0, q[3] * 0 - q[0] * 0 - q[1] * 1 - q[2] * 0]
    starts[7] = 0.0
    starts[8, 5] = np.nan
    starts[9, :4] = 0.0
    starts[10, 2] = np.inf
    return dict(X=X, m=m, offsets=np.array(offsets, np.int32), mask=mask, starts=starts, names=names, rows=rows)


@pytest.mark.parametrize("stride", (7, 12))
def test_degenerate_ranges_and_starts(ctx, oracle, stride):
    d = _degenerate(oracle)
    starts = d["starts"]
    if stride == 12:
        starts = np.array([pc.model_of_pose(s) if np.isfinite(s).all() and s[:4].any() else np.zeros(12) for s in d["starts"]])
        starts[8] = pc.model_of_pose(d["starts"][0])
        starts[8, 10] = np.nan
        starts[10] = pc.model_of_pose(d["starts"][0])
        starts[10, 1] = -np.inf
        expect_start = [np.array(pr.pose_from_model(s.tolist())[0]) for s in starts]
    else:
        expect_start = list(d["starts"])
    min_rows = 6
    got = _refine(ctx, d["X"], d["m"], d["offsets"], starts, mask=d["mask"], min_rows=min_rows, info=True)
    term = got["summaries"]["termination"].tolist()
    want_inlier = np.full(d["rows"], pc.FILL_BYTE, np.uint8)
    for p, name in enumerate(d["names"]):
        lo, hi = int(d["offsets"][p]), int(d["offsets"][p + 1])
        valid = 0 <= lo < hi <= d["rows"]
        rows = np.arange(lo, hi)[d["mask"][lo:hi] != 0] if valid else np.arange(0)
        sm = got["summaries"][p]
        if name in ("zero_start", "nan_start", "zero_quaternion", "inf_start"):
            assert term[p] == NO_START, name
            assert got["summaries"][p:p + 1].tobytes() == np.array([(0, 0, NO_START, 0, 0.0, 0.0)], got["summaries"].dtype).tobytes(), name
            assert not got["poses"][p].any() and not got["info"][p].any() and got["n_inliers"][p] == 0, name
            want_inlier[lo:hi] = 0
            continue
        if len(rows) < min_rows:  # empty, zero_mask, four_rows, past_the_arrays, reversed
            assert term[p] == TOO_FEW, name
            assert got["poses"][p].tobytes() == expect_start[p].tobytes(), (name, got["poses"][p], expect_start[p])
            assert (sm["iterations"], sm["accepted"], sm["n_used"]) == (0, 0, len(rows)), name
            assert sm["initial_cost"] == 0.0 and sm["final_cost"] == 0.0 and not got["info"][p].any(), name
        else:  # regular, behind
            s = _same_as_single_call(ctx, got, p, d["X"][rows], d["m"][rows], expect_start[p], 63, 0.01, 50, True, name)
            if name == "behind":  # nothing in front of the camera: no cost, no gradient, the start comes back
                assert (s.iterations, s.termination, s.final_cost) == (0, 2, 0.0)
                assert got["poses"][p].tobytes() == expect_start[p].tobytes()
        if valid:  # classified under the pose written, TOO_FEW included
            want = pr.classify(got["poses"][p].tolist(), d["X"][lo:hi].tolist(), d["m"][lo:hi].tolist(), pc.INLIER_THRESHOLD)
            want_inlier[lo:hi] = want
            assert got["n_inliers"][p] == sum(want), name
            assert name != "behind" or sum(want) == 0
        else:
            assert got["n_inliers"][p] == 0, name
    assert got["inlier"].tobytes() == want_inlier.tobytes()
    assert term[0] in (0, 1, 2) and got["n_inliers"][0] > 50
    if stride == 12:  # the conversion on the device is the restated one (TOO_FEW hands it out untouched)
        assert got["poses"][3].tobytes() == expect_start[3].tobytes() and got["poses"][3].any()


def test_all_rows_masked_without_a_floor_equals_the_single_call_on_no_rows(ctx, oracle):
    d = _degenerate(oracle)
    got = _refine(ctx, d["X"], d["m"], d["offsets"], d["starts"], mask=d["mask"], nproblems=3, min_rows=0)
    _same_as_single_call(ctx, got, 2, d["X"][:0], d["m"][:0], d["starts"][2], 63, 0.01, 50, True, "zero_mask")
    _same_as_single_call(ctx, got, 1, d["X"][:0], d["m"][:0], d["starts"][1], 63, 0.01, 50, True, "empty")


def test_refusals(ctx, oracle):
    """nproblems == 0 is GH_OK; every argument error returns GH_ERR_ARG without a launch (the dirty buffers stay dirty)."""
    import torch
    from gslam_amd import hip
    b = pc.census(oracle)
    n, rows = 4, len(b["X"])
    X, m, off, st, mask = _dev(b["X"]), _dev(b["m"]), _dev(b["offsets"][:n + 1]), _dev(b["starts"][:n]), _dev(b["mask"])
    out = _dirty(n, rows)
    opt = _options(0.01, 5)
    nan = float("nan")

    def call(ctxh=ctx.h, X=X, m=m, off=off, n=n, rows=rows, st=st, stride=7, min_rows=0, thr=0.01, drop=None):
        o = [None if k == drop else _ptr(out[k]) for k in OUT]
        return hip.lib.gh_pnp_refine_batch_dev(ctxh, _ptr(X), _ptr(m), _ptr(off), n, rows, _ptr(mask), _ptr(st), stride, 63,
                                               C.byref(opt), min_rows, C.c_double(thr), *o)

    bad = [dict(ctxh=None), dict(X=None), dict(m=None), dict(off=None), dict(st=None), dict(n=-1), dict(rows=-1), dict(stride=6),
           dict(stride=9), dict(stride=0), dict(min_rows=-1), dict(thr=nan), dict(drop="poses"), dict(drop="summaries")]
    for kw in bad:
        assert call(**kw) == GH_ERR_ARG, kw
    assert call(n=0) == 0 and call(n=0, X=None, st=None) == 0

    models = torch.full((n, 12), pc.FILL_DOUBLE, dtype=torch.float64, device="cuda")
    rin = torch.full((n,), pc.FILL_INT, dtype=torch.int32, device="cuda")
    sums2 = torch.full((n, 2, 32), pc.FILL_BYTE, dtype=torch.uint8, device="cuda")

    def chain(ctxh=ctx.h, X=X, off=off, n=n, rows=rows, rthr=0.01, thr=0.01, min_rows=0, models=models, rin=rin, poses=out["poses"],
              sums=sums2):
        return hip.lib.gh_pnp_batch_dev(ctxh, _ptr(X), _ptr(m), _ptr(off), n, rows, C.c_double(rthr), C.c_uint64(1), 63, C.byref(opt),
                                        min_rows, C.c_double(thr), _ptr(models), _ptr(rin), _ptr(poses), _ptr(out["info"]), _ptr(sums),
                                        _ptr(out["inlier"]), _ptr(out["n_inliers"]))

    for kw in (dict(ctxh=None), dict(X=None), dict(off=None), dict(n=-1), dict(rows=-1), dict(rthr=-1.0), dict(rthr=nan),
               dict(thr=-1.0), dict(thr=nan), dict(min_rows=-1), dict(models=None), dict(rin=None), dict(poses=None), dict(sums=None)):
        assert chain(**kw) == GH_ERR_ARG, kw
    assert chain(n=0) == 0
    torch.cuda.synchronize()
    assert (out["poses"].cpu().numpy() == pc.FILL_DOUBLE).all() and (out["inlier"].cpu().numpy() == pc.FILL_BYTE).all()
    assert (models.cpu().numpy() == pc.FILL_DOUBLE).all() and (sums2.cpu().numpy() == pc.FILL_BYTE).all()
    assert call() == 0  # the context is usable after a refusal
    torch.cuda.synchronize()
    assert (out["n_inliers"].cpu().numpy() >= 0).all()


PARITY = [(41, 200, 0.002, 7, 0.01, 63), (42, 1000, 0.002, 5, 0.01, 63), (43, 60, 0.004, 0, 0.0, 63),
          (44, 300, 0.002, 9, 0.01, 0b111000), (45, 300, 0.002, 9, 0.01, 0b000111)]  # of test_pnp_parity_noisy_huber


def test_oracle_parity_of_the_noisy_huber_sets(ctx, oracle):
    """The five sets as one batch without a mask.  One call fixes huber and dof for all its problems, so the batch is run
    once per distinct (huber, dof) and every problem is compared under its own."""
    cases = [pc.pnp_case(oracle, s, n, noise, every) for s, n, noise, every, _, _ in PARITY]
    X, m = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    offsets = np.cumsum([0] + [len(c[0]) for c in cases]).astype(np.int32)
    starts = np.array([c[2] for c in cases])
    runs = {}
    for p, (_, _, _, _, huber, dof) in enumerate(PARITY):
        if (huber, dof) not in runs:
            runs[huber, dof] = _refine(ctx, X, m, offsets, starts, dof=dof, huber=huber, max_iterations=50, info=True)
        got = runs[huber, dof]
        po, so, io, rc = oracle.ba_pnp(cases[p][0], cases[p][1], starts[p], dof=dof,
                                       opts=oracle_lib.ba_options(huber=huber, max_iterations=50), want_information=True)
        assert rc == 0
        sm = got["summaries"][p]
        print(PARITY[p], "pose %.3e cost %.3e info %.3e" % (np.abs(got["poses"][p] - po).max(), abs(sm["final_cost"] - so.final_cost) / so.final_cost,
                                                         np.abs(got["info"][p].reshape(6, 6) - io).max() / np.abs(io).max()))
        assert (sm["iterations"], sm["accepted"], sm["termination"]) == (so.iterations, so.accepted, so.termination)
        assert abs(sm["initial_cost"] - so.initial_cost) <= COST_RTOL * so.initial_cost
        assert abs(sm["final_cost"] - so.final_cost) <= COST_RTOL * so.final_cost
        assert np.abs(got["poses"][p] - po).max() <= STATE_ATOL
        assert np.abs(got["info"][p].reshape(6, 6) - io).max() <= 1e-9 * np.abs(io).max()
        assert so.final_cost < so.initial_cost


CHAIN_ROWS = (60, 110, 160, 200, 257, 300, 350, 400)
CHAIN_RANSAC_THR, CHAIN_THR, CHAIN_MIN_ROWS, CHAIN_SEED = 0.03, 0.004, 24, 12345


def _chain_inputs(oracle):
    """Eight regular problems (noise 0.002, every fifth observation displaced by 0.1), one of 5 rows (below the 6-point sample:
    no model) and one of 30 rows whose fit holds them all but whose refined pose keeps fewer than CHAIN_MIN_ROWS of them: 16
    of its observations are off by 0.012, inside the fit's threshold and outside the refinement's."""
    cases = [pc.pnp_case(oracle, 500 + i, n, 0.002, 5) for i, n in enumerate(CHAIN_ROWS)]
    X5, m5, _, _ = pc.pnp_case(oracle, 600, 5, 0.002, 0)
    X30, m30, _, _ = pc.pnp_case(oracle, 601, 30, 0.0003, 0)
    ang = np.arange(16) * (2 * np.pi * 5 / 16)
    m30 = m30.copy()
    m30[14:] += 0.012 * np.stack([np.cos(ang), np.sin(ang)], 1)
    X = np.concatenate([c[0] for c in cases] + [X5, X30])
    m = np.concatenate([c[1] for c in cases] + [m5, m30])
    disp = np.concatenate([c[3] for c in cases] + [np.zeros((35, 2))])
    offsets = np.cumsum([0] + [len(c[0]) for c in cases] + [5, 30]).astype(np.int32)
    return X, m, offsets, disp


def test_chain_equals_the_three_public_calls(ctx, oracle):
    import torch
    from gslam_amd import estimator, hip
    X, m, offsets, disp = _chain_inputs(oracle)
    P, rows = len(offsets) - 1, len(X)
    dX, dm, doff = _dev(X), _dev(m), _dev(offsets)
    opt = _options(0.01, 50)
    out = _dirty(P, rows)
    models = torch.full((P, 12), pc.FILL_DOUBLE, dtype=torch.float64, device="cuda")
    rin = torch.full((P,), pc.FILL_INT, dtype=torch.int32, device="cuda")
    sums = torch.full((P, 2, 32), pc.FILL_BYTE, dtype=torch.uint8, device="cuda")
    st = hip.lib.gh_pnp_batch_dev(ctx.h, _ptr(dX), _ptr(dm), _ptr(doff), P, rows, C.c_double(CHAIN_RANSAC_THR), C.c_uint64(CHAIN_SEED), 63,
                                  C.byref(opt), CHAIN_MIN_ROWS, C.c_double(CHAIN_THR), _ptr(models), _ptr(rin), _ptr(out["poses"]),
                                  _ptr(out["info"]), _ptr(sums), _ptr(out["inlier"]), _ptr(out["n_inliers"]))
    assert st == 0, hip.lib.gh_last_error(ctx.h)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ("poses", "info", "inlier", "n_inliers")}
    got.update(models=models.cpu().numpy(), ransac_inliers=rin.cpu().numpy(),
               summaries=sums.cpu().numpy().view(estimator.SUMMARY_DTYPE).reshape(P, 2))

    # the composition, through the mirror
    w_models, w_mask, w_rin = estimator.estimate_batch(ctx, estimator.PNP, dX, dm, doff, CHAIN_RANSAC_THR, CHAIN_SEED)
    r1 = estimator.pnp_refine_batch(ctx, dX, dm, doff, w_models, mask=w_mask, options=opt, min_rows=CHAIN_MIN_ROWS,
                                    inlier_threshold=CHAIN_THR)
    r2 = estimator.pnp_refine_batch(ctx, dX, dm, doff, r1["poses"], mask=r1["inlier"], options=opt, min_rows=CHAIN_MIN_ROWS,
                                    inlier_threshold=CHAIN_THR, want_information=True)
    torch.cuda.synchronize()
    assert r1["info"] is None
    s1 = r1["summaries"].cpu().numpy().view(estimator.SUMMARY_DTYPE).reshape(P)
    s2 = r2["summaries"].cpu().numpy().view(estimator.SUMMARY_DTYPE).reshape(P)
    want = dict(models=w_models.cpu().numpy(), ransac_inliers=w_rin.cpu().numpy(), poses=r2["poses"].cpu().numpy(),
                info=r2["info"].cpu().numpy(), inlier=r2["inlier"].cpu().numpy(), n_inliers=r2["n_inliers"].cpu().numpy(),
                summaries=np.stack([s1, s2], 1))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    # the mirror of the chain makes the same call
    mirror = estimator.pnp_batch(ctx, dX, dm, doff, CHAIN_RANSAC_THR, CHAIN_SEED, CHAIN_THR, options=opt, min_rows=CHAIN_MIN_ROWS,
                                 want_information=True)
    torch.cuda.synchronize()
    for k in ("models", "ransac_inliers", "poses", "info", "inlier", "n_inliers"):
        assert mirror[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert mirror["summaries"].cpu().numpy().tobytes() == want["summaries"].tobytes()

    term = got["summaries"]["termination"]
    print("chain: ransac inliers", got["ransac_inliers"].tolist(), "round-1 inliers", r1["n_inliers"].cpu().numpy().tolist(),
          "final", got["n_inliers"].tolist(), "termination", term.tolist())
    # 5 rows: no model, no start in both rounds, everything zero
    assert got["ransac_inliers"][8] == 0 and term[8].tolist() == [NO_START, NO_START]
    assert not got["poses"][8].any() and not got["inlier"][offsets[8]:offsets[9]].any() and got["n_inliers"][8] == 0
    # 30 rows: the first round is optimised, its inliers are fewer than min_rows, the second round keeps the first fit
    assert got["ransac_inliers"][9] >= CHAIN_MIN_ROWS and 0 <= term[9, 0] <= 3 and term[9, 1] == TOO_FEW
    assert got["summaries"][9, 1]["n_used"] < CHAIN_MIN_ROWS
    assert got["poses"][9].tobytes() == r1["poses"].cpu().numpy()[9].tobytes()
    # the regular problems
    p1, in1 = r1["poses"].cpu().numpy(), r1["inlier"].cpu().numpy()
    for p in range(8):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        assert (term[p] <= 3).all() and got["n_inliers"][p] > 0.6 * (hi - lo), p
        far = np.hypot(disp[lo:hi, 0], disp[lo:hi, 1]) > CHAIN_THR
        assert far.sum() >= (hi - lo) // 5 - 2 and not got["inlier"][lo:hi][far].any(), p
        rows = np.arange(lo, hi)[in1[lo:hi] != 0]
        po, so, _, rc = oracle.ba_pnp(X[rows], m[rows], p1[p], opts=oracle_lib.ba_options(huber=0.01, max_iterations=50))
        assert rc == 0 and np.abs(got["poses"][p] - po).max() <= STATE_ATOL, (p, np.abs(got["poses"][p] - po).max())
