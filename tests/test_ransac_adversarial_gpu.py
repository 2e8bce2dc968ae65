"""GPU parity of gh_ransac_estimate_ex / gh_triangulate with oracle/ransac_oracle.c on the adversarial classes of
tests/ransac_cases.py (tests/test_ransac_adversarial_oracle.py shows on the CPU that each class reaches the branch it
names): model doubles, inlier mask, inlier count and hypotheses_used equal the oracle's bit for bit, in all three
sampling modes.  No case can hang a kernel: every call passes n rows with n-row arrays, and the rejection sampler ends
for every n >= s (smaller n return before any launch)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac_cases as rc

pytestmark = pytest.mark.gpu

MODES = (rc.RANSAC, rc.LMEDS, rc.NOSAMPLE)
SEED = 3
GH_ERR_ARG = 1  # include/gslam_hip.h


def _same(got, want, key):
    gm, gmask, gcnt, gused = got
    em, emask, ecnt, eused = want
    assert (gcnt, gused) == (ecnt, eused), (key, gcnt, ecnt, gused, eused)
    assert np.array_equal(gmask, emask), (key, int(gmask.sum()), int(emask.sum()))
    assert gm.tobytes() == em.tobytes(), (key, gm, em)


def _parity(ctx, oracle, model, P, Q, thr, samp, key, confidence=1.0, seed=SEED):
    from gslam_amd import estimator
    want = oracle.estimate_ex(model, P, Q, thr, samp, confidence=confidence, seed=seed)
    got = estimator.estimate_ex(ctx, model, P, Q, thr, samp, confidence=confidence, seed=seed)
    _same(got, want, key)
    return want


@pytest.mark.parametrize("name", list(rc.CLASSES))
def test_class_parity(ctx, oracle, name):
    from gslam_amd import estimator
    ran = 0
    for model in rc.MODELS:
        c = rc.CLASSES[name](model, 0)
        if c is None:
            continue
        P, Q, thr, expect = c
        for samp in MODES:
            _parity(ctx, oracle, model, P, Q, thr, samp, (name, model, samp))
            ran += 1
        for conf in (0.5, 0.99, 1.0):
            want = oracle.ransac_conf(model, P, Q, thr, conf, seed=SEED)
            got = estimator.estimate_conf(ctx, model, P, Q, thr, conf, seed=SEED)
            _same(got, want, (name, model, "conf", conf))
    assert ran


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_estimator_seeds(ctx, oracle, seed):
    for model in rc.MODELS:
        P, Q, thr, _ = rc.CLASSES["nominal"](model, 0)
        for samp in (rc.RANSAC, rc.LMEDS):
            _parity(ctx, oracle, model, P, Q, thr, samp, (seed, model, samp), confidence=0.99, seed=seed)


@pytest.mark.parametrize("samp", MODES)
def test_large_parity(ctx, oracle, samp):
    model, P, Q, thr, expect = rc.large(samp)
    assert len(P) > 65536
    want = _parity(ctx, oracle, model, P, Q, thr, samp, ("large", samp))
    assert want[2] > len(P) // 2 or samp == rc.NOSAMPLE  # (least squares over 28 % outliers fits few rows)
    assert want[0].any()


def _no_model_cases():
    for name, model, P, Q, thr, expect in rc.cases():
        for samp in MODES:
            if rc.expect_for(expect, samp) in ("no_model", "median_inf", "projection"):
                yield name, model, samp, P, Q, thr


def test_no_model_contract(ctx):
    """0 inliers means no model (include/gslam_hip.h): then the model is all zero AND the caller's mask is all zero, also
    where a winner was scored and copied out before its essential projection failed.  The mask goes in dirty."""
    from gslam_amd import hip
    seen = set()
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, model, samp, P, Q, thr in _no_model_cases():
        n = len(P)
        m = np.full(12, 7.0)
        mask = np.full(max(n, 1), 0xAB, np.uint8)
        cnt, used = C.c_int(-5), C.c_int(-5)
        st = hip.lib.gh_ransac_estimate_ex(ctx.h, model, pv(P), pv(Q), n, C.c_double(thr), C.c_double(1.0), C.c_uint64(SEED), samp,
                                           pv(m), pv(mask), C.byref(cnt), C.byref(used))
        assert st == 0, (name, model, samp, st)
        assert cnt.value == 0 and not m.any() and not mask[:n].any(), (name, model, samp, cnt.value, int(mask[:n].sum()))
        seen.add(name)
    assert {"projection_failure", "projection_underflow", "collinear", "coincident", "n_s_minus_1", "nonfinite_majority"} <= seen


def _sequence_cases():
    P, Q, thr, _ = rc.CLASSES["nominal"](0, 0)
    yield "nominal", 0, P, Q, thr
    P, Q, thr, _ = rc.CLASSES["coincident"](1, 0)
    yield "no_model", 1, P, Q, thr
    P, Q, thr, _ = rc.CLASSES["projection_underflow"](4, 0)
    yield "projection", 4, P, Q, thr


def test_mask_is_optional(ctx):
    """mask_out = NULL: the same model, count and hypotheses_used as with a mask, in all three sampling modes."""
    from gslam_amd import estimator, hip
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, model, P, Q, thr in _sequence_cases():
        for samp in MODES:
            wm, wmask, wcnt, wused = estimator.estimate_ex(ctx, model, P, Q, thr, samp, seed=SEED)
            m = np.full(12, 7.0)
            cnt, used = C.c_int(-5), C.c_int(-5)
            st = hip.lib.gh_ransac_estimate_ex(ctx.h, model, pv(P), pv(Q), len(P), C.c_double(thr), C.c_double(1.0),
                                               C.c_uint64(SEED), samp, pv(m), None, C.byref(cnt), C.byref(used))
            assert st == 0 and (cnt.value, used.value) == (wcnt, wused) and m.tobytes() == wm.tobytes(), (name, samp)
            assert (wcnt > 0) == (name == "nominal") or samp == rc.NOSAMPLE, (name, samp, wcnt)


def test_call_sequence_independence(ctx, oracle):
    """Scratch and pinned blocks are reused and only partly overwritten: a large call, a tiny one, a no-model one and
    the first again return identical bytes each time, in every mode."""
    from gslam_amd import estimator
    Pl, Ql, thrl = rc.nominal(1, 70001)
    Pt, Qt, thrt = rc.nominal(1, 3)
    Pn, Qn, thrn, _ = rc.CLASSES["coincident"](1, 0)
    Pe, Qe, thre, _ = rc.CLASSES["projection_underflow"](4, 0)
    for samp in MODES:
        seq = [(1, Pl, Ql, thrl), (1, Pt, Qt, thrt), (1, Pn, Qn, thrn), (4, Pe, Qe, thre), (1, Pl, Ql, thrl), (1, Pt, Qt, thrt)]
        out = [estimator.estimate_ex(ctx, mo, P, Q, thr, samp, seed=SEED) for mo, P, Q, thr in seq]
        for a, b in ((0, 4), (1, 5)):
            _same(out[a], out[b], (samp, a, b))
        if samp != rc.LMEDS:  # (the oracle's LMedS at 70 001 rows takes a quarter of a minute: test_large_parity has it once)
            _same(out[0], oracle.estimate_ex(1, Pl, Ql, thrl, samp, seed=SEED), (samp, "large"))
        _same(out[1], oracle.estimate_ex(1, Pt, Qt, thrt, samp, seed=SEED), (samp, "tiny"))
        _same(out[2], oracle.estimate_ex(1, Pn, Qn, thrn, samp, seed=SEED), (samp, "no model"))
        _same(out[3], oracle.estimate_ex(4, Pe, Qe, thre, samp, seed=SEED), (samp, "projection"))
        assert not out[2][1].any() and not out[3][1].any() and not out[3][0].any()


def test_refusals(ctx):
    """Argument checks the entry makes itself: wrong model, wrong sampling, negative or NaN threshold; n < s is no error."""
    from gslam_amd import hip
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    P, Q, thr = rc.nominal(0, 50)

    def call(model, samp, t, n=50):
        m, mask = np.full(12, 7.0), np.full(64, 0xAB, np.uint8)
        cnt, used = C.c_int(-5), C.c_int(-5)
        st = hip.lib.gh_ransac_estimate_ex(ctx.h, model, pv(P), pv(Q), n, C.c_double(t), C.c_double(1.0), C.c_uint64(1), samp,
                                           pv(m), pv(mask), C.byref(cnt), C.byref(used))
        return st, m, mask, cnt.value, used.value

    assert call(0, 0, thr)[0] == 0
    for model, samp, t in ((-1, 0, thr), (8, 0, thr), (0, 3, thr), (0, -1, thr), (0, 0, -1.0), (0, 0, float("nan")), (0, 1, -0.5)):
        st = call(model, samp, t)[0]
        assert st == GH_ERR_ARG, (model, samp, t, st)
    for samp in MODES:
        st, m, mask, cnt, used = call(0, samp, thr, n=3)
        assert st == 0 and cnt == 0 and used == 0 and not m.any() and not mask[:3].any()
    assert call(0, 0, thr)[0] == 0  # the context is usable after a refusal


def test_triangulate_edges(ctx, oracle):
    from gslam_amd import estimator
    from gslam_amd.ba_synth import _quat_from_R
    from test_ransac_oracle import _rot
    assert estimator.triangulate(ctx, np.zeros(7), np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 3)
    for n in (1, 255, 257, 70001):
        rng = np.random.default_rng(n)
        R, t = _rot([0.1, 1, 0.2], 0.2), np.array([-0.8, 0.02, 0.05])
        pose = np.r_[_quat_from_R(R[None])[0], t]
        X = np.c_[rng.uniform(-2, 2, (n, 2)), rng.uniform(3, 10, n)]
        d1 = X / X[:, 2:3]
        X2 = X @ R.T + t
        d2 = X2 / X2[:, 2:3]
        poses = np.tile(pose, (n, 1))
        k = np.arange(n) % 16
        d1[k == 1] = 0.0                                # zero-length direction
        d2[k == 2] = 0.0
        d2[k == 3] = d1[k == 3] @ R.T                   # exactly parallel rays
        d1[k == 4, rng.integers(0, 3)] = np.nan         # NaN rows
        d2[k == 5] = np.inf
        d2[k == 6] = -d2[k == 6]                        # behind the current camera
        d1[k == 7] = -d1[k == 7]                        # behind the reference camera
        d1[k == 8, 0] -= 3.0                            # diverging
        poses[k == 9, 4:] += rng.normal(size=(int((k == 9).sum()), 3))  # per-row poses that differ
        poses[k == 10, :4] = 0.0                        # a zero quaternion: R = I
        got1, ok1 = estimator.triangulate(ctx, pose, d1, d2)
        gotn, okn = estimator.triangulate(ctx, poses, d1, d2)
        step = 1 if n < 1000 else 7
        for i in list(range(0, n, step)) + [n - 1]:
            e, eok = oracle.triangulate(pose, d1[i], d2[i])
            assert eok == ok1[i] and e.tobytes() == got1[i].tobytes(), (n, i, "one pose")
            e, eok = oracle.triangulate(poses[i], d1[i], d2[i])
            assert eok == okn[i] and e.tobytes() == gotn[i].tobytes(), (n, i, "per-row poses")
        if n >= 255:
            assert 0 < ok1.sum() < n and not ok1[(k >= 1) & (k <= 7)].any()


def test_fuzz(ctx, oracle):
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=80, deadline=None, derandomize=True, database=None)
    @given(model=st.integers(0, 7), samp=st.sampled_from(MODES), n=st.integers(3, 700), outliers=st.sampled_from([0.0, 0.1, 0.3, 0.6, 0.9]),
           noisy=st.booleans(), integer=st.booleans(), exp=st.integers(-6, 6), nan_rows=st.sampled_from([0, 0, 3]),
           conf=st.sampled_from([0.5, 0.99, 1.0]), seed=st.integers(0, 2 ** 64 - 1), data_seed=st.integers(0, 50))
    def run(model, samp, n, outliers, noisy, integer, exp, nan_rows, conf, seed, data_seed):
        rng = np.random.default_rng([model, n, data_seed])
        P, Q, thr = rc.nominal(model, n, data_seed)
        f = 10.0 ** exp
        if model not in (4, 7):
            P, Q, thr = P * f, Q * f, thr * f
        elif model == 7:
            P = P * f
        bad = rng.random(n) < outliers
        Q[bad] += rng.uniform(-50, 50, (int(bad.sum()), Q.shape[1])) * thr
        if noisy:
            Q += rng.normal(size=Q.shape) * 0.2 * thr
        if integer:
            P, Q, thr = np.round(P / thr), np.round(Q / thr), 1.0
        for r in rng.choice(n, min(nan_rows, n), replace=False):
            (P if r % 2 else Q)[r, 0] = np.nan
        if model == 6:
            Q = P.copy()
        _parity(ctx, oracle, model, P, Q, thr, samp, (model, samp, n, exp, seed), confidence=conf, seed=seed)

    run()


# ---------------------------------------------------------------- through the GSLAM plugin
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "oracle", "_ref", "bin", "plugin_host")
PLUGDIR = os.path.join(ROOT, "oracle", "_ref", "plugins")


def _plugin_blocks(tmp_path, model, P, Q, thr):
    """plugin_host est -> [(ok, mask)] of the RANSAC, NOSAMPLE and LMEDS calls (LMEDS is not made for model 2)."""
    fin, out = tmp_path / "pts.raw", tmp_path / "out.bin"
    np.ascontiguousarray(np.c_[P, Q], dtype=np.float64).tofile(fin)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "gslam_amd", "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([HOST, "est", PLUGDIR, str(model), str(len(P)), str(fin), repr(float(thr)), str(out)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode in (0, 3), r.stdout + r.stderr  # 3: the first call found no model, which is what is asked here
    raw = open(out, "rb").read()
    blocks, o = [], 0
    for _ in range(3):
        ok, nm = struct.unpack_from("2i", raw, o)
        blocks.append((ok, np.frombuffer(raw, np.uint8, nm, o + 80)))
        o += 80 + nm
    return blocks


def test_plugin_degenerate_and_nan(tmp_path, oracle):
    """The plugin sizes and fills the caller's std::vector<uchar>: on "no model" it is n zeros, also behind a failed
    essential projection (the RANSAC call at confidence 0.99, then `| NOSAMPLE`, then bare LMEDS)."""
    if not (os.path.exists(HOST) and os.path.exists(os.path.join(PLUGDIR, "libgslam_estimator.so"))):
        pytest.skip("oracle/_ref/bin/plugin_host or libgslam_estimator.so missing: `make plugins` builds them where the GSLAM headers are")
    todo = []
    for model in (0, 2):
        todo.append((model,) + rc.CLASSES["coincident"](model, 0)[:3])
        P, Q, thr, _ = rc.CLASSES["nominal"](model, 0)
        Q[:, 0] = np.nan  # every row undefined: nobody can be an inlier
        todo.append((model, P, Q, thr))
    todo.append((4,) + rc.CLASSES["projection_underflow"](4, 0)[:3])
    todo.append((4,) + rc.CLASSES["projection_failure"](4, 0)[:3])
    for model, P, Q, thr in todo:
        blocks = _plugin_blocks(tmp_path, model, P, Q, thr)
        checked = 0
        for (ok, mask), samp in zip(blocks, (rc.RANSAC, rc.NOSAMPLE, rc.LMEDS)):
            if samp == rc.LMEDS and model in (2, 4):
                continue  # (LMEDS == F8_Point numerically: not a sampling flag for the two-view models)
            ecnt = oracle.estimate_ex(model, P, Q, thr, samp, confidence=0.99, seed=1)[2]
            if ecnt == 0:
                assert ok == 0 and len(mask) == len(P) and not mask.any(), (model, samp, ok, len(mask), int(mask.sum()))
                checked += 1
        assert checked, model  # every one of them is a no-model case in at least one of the calls
