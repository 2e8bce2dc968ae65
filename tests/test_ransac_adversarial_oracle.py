"""CPU: the adversarial estimator classes of tests/ransac_cases.py do what they claim (the census), and
oracle/ransac_oracle.c agrees with a restatement it shares no code with.

The restatement (numpy, np.longdouble for the errors): the eight error functions from their definitions -- forward
transfer error (H), residual of the affine map (A2, A3), Sampson distance (F, E), similarity residual with the rotation
applied as a quaternion sandwich (SIM3), point-plane distance, reprojection error with positive depth (PnP) -- and the
splitmix64 sample drawing from the comment at the top of gslam_amd/csrc/ransac.hip.  The linear models of the exact-tie
classes are solved with numpy.linalg, which pins the tie rules (lowest index among the best) without the oracle.

Mask check.  Whenever a model comes back, mask == (err <= thr2) row for row and count == popcount(mask), thr2 being
threshold^2 (RANSAC, NOSAMPLE) or the LMedS radius^2 restated from np.sort(err)[n // 2].  Rows whose restated error lies
within a relative band of thr2 are left out.  Measured over all classes, models and modes (the 636 cases in which a
finite model comes back; left aside are only F / E under NOSAMPLE on the coincident class, one point repeated, where
the Sampson distance is 0 / 0): oracle and restatement disagree on NO row, so the smallest agreeing band is 0, ten times
it is 0 as well, and no row is left out: 0 % in every class (the limit is 0.5 % of a case's rows; the exact-tie and
quantised classes may leave out none).  thr2 == 0 (threshold 0 or 1e-300) leaves no relative band: on the exact
classes the comparison is complete; on real-valued data a binary64 zero is a rounding accident of the sample's own rows,
so there the check is the implication mask -> err <= (2^-40 scale)^2, and its converse on the rows whose restated error
is exactly 0.
Model 4 returns the PROJECTED matrix with the mask of the unprojected 8-point estimate: its mask is compared with that of
model 2 on the same data (same draws, same solver, same scores), and the matrix with U diag(s, s, 0) V^T, s = (s1 + s2) /
2, from numpy's SVD of model 2's answer.

Oracle times behind ransac_cases.LARGE_N (one call, 2048 hypotheses, one thread of an idle x86 machine, A2 / plane):
  RANSAC   n = 65 537: 0.42 / 0.40 s   100 003: 0.71 / 0.58 s   200 003: 1.29 / 1.10 s   -> 200 003 (A2)
  LMedS    n = 65 537: 18.7 / 14.5 s   100 003: 25.4 / 20.9 s   200 003: 55.8 / 39.6 s   -> none is under 10 s; 65 537 (plane)
  NOSAMPLE one fit and one scoring pass, milliseconds at every size                        -> 200 003 (A2)"""
import numpy as np
import pytest

import ransac_cases as rc

LD = np.longdouble
BAND_MEASURED = 0.0   # no row of any case falls on the other side of thr2 in the oracle's binary64
BAND = 10 * BAND_MEASURED
LEFT_OUT_LIMIT = 0.005

M64 = (1 << 64) - 1
K_HYP = 2048
K_TINY = 1e-12


# ---------------------------------------------------------------- restatement: sampler
def _sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_sample(seed, h, n, s):
    """The s distinct row indices of hypothesis h: splitmix64 started at seed ^ h * 0xD1B5..., one value per attempt,
    value mod n, duplicates rejected."""
    st = _sm64((seed ^ (h * 0xD1B54A32D192ED03)) & M64)
    idx = []
    while len(idx) < s:
        st = _sm64(st)
        c = st % n
        if c not in idx:
            idx.append(c)
    return idx


# ---------------------------------------------------------------- restatement: errors
def restated_errors(model, m, P, Q):
    """Squared error of every row under model m (12 doubles), longdouble; undefined and NaN errors are +inf."""
    m = np.asarray(m, LD)
    P, Q = np.asarray(P, LD), np.asarray(Q, LD)
    n = len(P)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if model == 0:
            H = m[:9].reshape(3, 3)
            ph = np.c_[P, np.ones(n, LD)] @ H.T
            ok = np.abs(ph[:, 2]) > K_TINY
            d = ph[:, :2] / ph[:, 2:3] - Q
        elif model == 1:
            A = m[:6].reshape(2, 3)
            d = P @ A[:, :2].T + A[:, 2] - Q
        elif model == 3:
            A = m[:12].reshape(3, 4)
            d = P @ A[:, :3].T + A[:, 3] - Q
        elif model in (2, 4):
            F = m[:9].reshape(3, 3)
            x1, x2 = np.c_[P, np.ones(n, LD)], np.c_[Q, np.ones(n, LD)]
            Fx, Ftx = x1 @ F.T, x2 @ F
            num = np.sum(x2 * Fx, axis=1)
            den = Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2
            ok = den > 1e-300
            e = num * num / den
            e[~ok | np.isnan(e)] = np.inf
            return e
        elif model == 5:
            qv, qw, t, s = m[:3], m[3], m[4:7], m[7]
            c1 = np.cross(np.broadcast_to(qv, P.shape), P)
            rot = P + 2 * qw * c1 + 2 * np.cross(np.broadcast_to(qv, P.shape), c1)  # q (0, x) q* for a unit quaternion
            d = s * rot + t - Q
        elif model == 6:
            d = (P @ m[:3] + m[3])[:, None]
        else:
            R, t = m[:9].reshape(3, 3), m[9:12]
            Xc = P @ R.T + t
            ok = Xc[:, 2] > K_TINY
            d = Xc[:, :2] / Xc[:, 2:3] - Q
        e = np.sum(d * d, axis=1)
    e[~ok | np.isnan(e)] = np.inf
    return e


def _solve_linear(model, P, Q, idx):
    """The model through the sample rows by numpy.linalg (A2, A3, H) or the cross product (plane); None if singular."""
    p, q = P[idx], Q[idx]
    out = np.zeros(12)
    try:
        if model == 1:
            M = np.c_[p, np.ones(3)]
            if abs(np.linalg.det(M)) < 1e-9:
                return None
            out[:6] = np.linalg.solve(M, q).T.reshape(-1)
        elif model == 3:
            M = np.c_[p, np.ones(4)]
            if abs(np.linalg.det(M)) < 1e-9:
                return None
            out[:12] = np.linalg.solve(M, q).T.reshape(-1)
        elif model == 0:
            rows, rhs = [], []
            for (x, y), (u, v) in zip(p, q):
                rows += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
                rhs += [u, v]
            M = np.array(rows)
            if np.linalg.cond(M) > 1e10:
                return None
            out[:8] = np.linalg.solve(M, np.array(rhs))
            out[8] = 1.0
        else:
            nv = np.cross(p[1] - p[0], p[2] - p[0])
            ln = np.sqrt(nv @ nv)
            if not ln > K_TINY:
                return None
            nv = nv / ln
            out[:3], out[3] = nv, -(nv @ p[0])
    except np.linalg.LinAlgError:
        return None
    return out


def _restated_hypotheses(model, P, Q, seed):
    n, s = len(P), rc.S_OF[model]
    for h in range(K_HYP):
        m = _solve_linear(model, P, Q, draw_sample(seed, h, n, s))
        if m is not None:
            yield h, m, restated_errors(model, m, P, Q)


def _lmeds_thr2(err, thr, n, s):
    med = np.sort(err)[n // 2]
    sigma = LD(2.5) * LD(1.4826) * (1 + LD(5) / max(n - s, 1)) * np.sqrt(med)
    return max(LD(thr), sigma) ** 2


EXACT = ("ties_thr_0", "ties_thr_half", "ties_all_inliers", "ties_two_structures_thr_0", "ties_two_structures_thr_half", "quantised_odd", "quantised_even", "quantised_median_zero",
         "quantised_denormal")
SEED = 3


@pytest.fixture(scope="module")
def results(oracle):
    """Every class x model x sampling mode through the oracle, once."""
    out = {}
    for name, model, P, Q, thr, expect in rc.cases():
        for samp in (rc.RANSAC, rc.LMEDS, rc.NOSAMPLE):
            out[name, model, samp] = (P, Q, thr, rc.expect_for(expect, samp)) + oracle.estimate_ex(model, P, Q, thr, samp, seed=SEED)
    return out


# ---------------------------------------------------------------- census
def test_every_class_applies_somewhere_and_every_model_is_covered():
    seen = {}
    for name, model, P, Q, thr, expect in rc.cases():
        seen.setdefault(name, []).append(model)
        assert P.shape == (len(P), rc.DIM_P[model]) and Q.shape == (len(P), rc.DIM_Q[model]) and thr >= 0
    assert set(seen) == set(rc.CLASSES)
    for name in ("nominal", "coincident", "collinear", "five_distinct", "s_distinct_good", "n_s_plus_0", "block_257",
                 "nonfinite_both", "thr_0", "thr_inf"):
        assert seen[name] == list(rc.MODELS), name
    for n in (63, 64, 65, 255, 256, 257, 511, 513):
        assert "block_%d" % n in seen
    assert min(rc.LARGE_N.values()) > 65536


def test_census_each_class_reaches_the_branch_it_names(oracle, results):
    reached = {}
    for (name, model, samp), (P, Q, thr, expect, m, mask, cnt, used) in results.items():
        n, s, key = len(P), rc.S_OF[model], (name, model, samp)
        assert cnt == int(mask.sum()), key
        assert used == (0 if n < s else (K_HYP if samp != rc.NOSAMPLE else used)), key
        reached[expect] = reached.get(expect, 0) + 1
        if expect == "no_model":
            assert cnt == 0 and not m.any() and not mask.any(), key
        elif expect == "model":
            assert cnt >= s and m.any() and np.isfinite(m).all(), (key, cnt)
        elif expect == "median_inf":
            assert samp == rc.LMEDS and cnt == 0 and not m.any() and not mask.any(), key
            # the same rows with a fifth of them bad instead of 55 %: a model comes back
            assert results["nonfinite_fifth", model, samp][6] >= s, key
            assert results[name, model, rc.RANSAC][6] >= s, key  # and RANSAC still finds one in the majority case
        elif expect == "projection":
            assert model == 4 and cnt == 0 and not m.any() and not mask.any(), key
            fm, fmask, fcnt, _ = oracle.estimate_ex(2, P, Q, thr, samp, seed=SEED)  # the unprojected winner scores inliers
            assert fcnt >= 8 and fm.any(), (key, fcnt)
            sv = np.linalg.svd(fm[:9].reshape(3, 3).astype(np.float64), compute_uv=False)
            assert not sv[1] ** 2 > 1e-300, (key, sv)  # rank 1 to within the floor of project_essential
        elif expect == "all_inliers":
            assert samp == rc.RANSAC and cnt == n, key
            # every valid hypothesis holds the maximum, so the confidence rule stops at the first of them (pg >= 1)
            cm, cmask, ccnt, cused = oracle.estimate_ex(model, P, Q, thr, samp, confidence=0.5, seed=SEED)
            assert ccnt == n and cused < 64 and cm.tobytes() == m.tobytes(), (key, cused)
        elif expect == "ties":  # test_tie_rule_* counts the hypotheses at the optimum: this case must be one of theirs
            assert (name, model) in {(c[0], c[1]) for c in _tie_cases(samp)}, key
        else:
            assert expect == "any", key
    for e in ("model", "no_model", "ties", "all_inliers", "median_inf", "projection", "any"):
        assert reached.get(e, 0) > 0, e
    # the projection failure is reached in all three modes (scale underflow) and by the exact construction (NOSAMPLE)
    assert all(results["projection_underflow", 4, sm][3] == "projection" for sm in (0, 1, 2))
    assert results["projection_failure", 4, rc.NOSAMPLE][3] == "projection"
    # at 1e-6 the absolute pivots refuse what the nominal scale accepts (H, NOSAMPLE: the normal equations)
    assert results["scale_1e-6", 0, rc.NOSAMPLE][7] == 0 and results["nominal", 0, rc.NOSAMPLE][7] == 1


# ---------------------------------------------------------------- restatement: masks and counts
def _mask_check(key, model, P, Q, thr2, m, mask, exact):
    """-> (rows left out, largest relative distance of a disagreeing row)."""
    err = restated_errors(model, m, P, Q)
    want = err <= thr2
    got = mask.astype(bool)
    if exact:
        assert np.array_equal(got, want), key
        return 0, 0.0
    if thr2 == 0:
        scale = float(np.nanmax(np.abs(np.where(np.isfinite(Q), Q, 0)))) + 1.0
        assert (err[got] <= (2.0 ** -40 * scale) ** 2).all(), key
        assert got[err == 0].all(), key  # and the converse where the restatement itself finds an exact zero
        return 0, 0.0
    if not np.isfinite(thr2):
        assert np.array_equal(got, want), key
        return 0, 0.0
    with np.errstate(all="ignore"):
        rel = np.abs(err - thr2) / thr2
    bad = got != want
    worst = float(rel[bad].max()) if bad.any() else 0.0
    out = (rel <= BAND) & (BAND > 0)  # (a band of 0 leaves out nothing: a row exactly on thr2 is an inlier on both sides)
    assert np.array_equal(got[~out], want[~out]), (key, worst)
    assert out.sum() <= LEFT_OUT_LIMIT * len(P), (key, int(out.sum()))
    return int(out.sum()), worst


def test_masks_and_counts_equal_the_restated_errors(oracle, results, capsys):
    worst_all, left = 0.0, {}
    checked = 0
    for (name, model, samp), (P, Q, thr, expect, m, mask, cnt, used) in results.items():
        key, n, s = (name, model, samp), len(P), rc.S_OF[model]
        if not m.any() or not np.isfinite(m).all():
            continue
        if (name, samp) == ("coincident", rc.NOSAMPLE) and model in (2, 4):
            continue  # one point repeated: x'^T F x and the gradient both vanish, the Sampson distance is 0 / 0 in any precision
        if model == 4:
            fm, fmask, fcnt, _ = oracle.estimate_ex(2, P, Q, thr, samp, seed=SEED)
            assert np.array_equal(mask, fmask) and cnt == fcnt, key
            U, sv, Vt = np.linalg.svd(fm[:9].reshape(3, 3))
            E = U @ np.diag([(sv[0] + sv[1]) / 2] * 2 + [0.0]) @ Vt
            assert np.abs(E - m[:9].reshape(3, 3)).max() <= 1e-7 * sv[0], key
            m_scored = fm
        else:
            m_scored = m
        err = restated_errors(model, m_scored, P, Q)
        thr2 = _lmeds_thr2(err, thr, n, s) if samp == rc.LMEDS else LD(thr) ** 2
        if samp != rc.LMEDS:
            with np.errstate(all="ignore"):
                thr2 = LD(np.float64(thr) * np.float64(thr))  # the oracle squares in binary64: 1e-300 -> 0, 1e200 -> +inf
        out, worst = _mask_check(key, model, P, Q, thr2, m_scored, mask, name in EXACT and samp != rc.NOSAMPLE)
        left[name] = max(left.get(name, 0.0), out / n)
        worst_all = max(worst_all, worst)
        checked += 1
    with capsys.disabled():
        print("\nmask restatement: %d cases, smallest agreeing band %.3e, left-out share per class (max): %s"
              % (checked, worst_all, {k: v for k, v in left.items() if v}))
    assert checked >= 630
    assert worst_all <= BAND_MEASURED


# ---------------------------------------------------------------- restatement: tie rules
def _tie_cases(expect_mode):
    for name, model, P, Q, thr, expect in rc.cases():
        if model in (0, 1, 3, 6) and rc.expect_for(expect, expect_mode) == "ties":
            yield name, model, P, Q, thr


def test_tie_rule_ransac_lowest_index_among_the_largest_counts(oracle):
    seen = observable = 0
    for name, model, P, Q, thr in _tie_cases(rc.RANSAC):
        counts = {h: int((err <= LD(thr) ** 2).sum()) for h, m, err in _restated_hypotheses(model, P, Q, SEED)}
        top = max(counts.values())
        at_top = sorted(h for h, c in counts.items() if c == top)
        assert len(at_top) >= 2, (name, model, top)
        hs = at_top[0]
        want = _solve_linear(model, P, Q, draw_sample(SEED, hs, len(P), rc.S_OF[model]))
        m, mask, cnt, used = oracle.estimate_ex(model, P, Q, thr, rc.RANSAC, seed=SEED)
        assert cnt == top and used == K_HYP, (name, model, cnt, top)
        assert np.allclose(m, want, rtol=1e-9, atol=1e-9), (name, model, hs)
        if name in EXACT:  # (equal as values: the plane's offset is -0.0 in the oracle)
            assert np.array_equal(m, want), (name, model)
        # a later hypothesis at the same count is a different sample, not necessarily a different model: the rule shows
        # only where one of them has a model the comparison above tells from the first one's
        models = {h: _solve_linear(model, P, Q, draw_sample(SEED, h, len(P), rc.S_OF[model])) for h in at_top}
        others = [h for h in at_top if not (np.array_equal(models[h], want) if name in EXACT else
                                            np.allclose(models[h], want, rtol=1e-9, atol=1e-9))]
        if name.startswith("ties_two_structures"):
            assert others, (name, model)
        if others:
            assert not np.array_equal(m, models[others[-1]]) and others[-1] > hs, (name, model, hs, others[-1])
            observable += 1
        seen += 1
        # the confidence rule looks at a prefix: its winner is the lowest index at the prefix's maximum
        cm, cmask, ccnt, cused = oracle.estimate_ex(model, P, Q, thr, rc.RANSAC, confidence=0.5, seed=SEED)
        pre = {h: c for h, c in counts.items() if h < cused}
        assert ccnt == max(pre.values()), (name, model)
        hp = min(h for h, c in pre.items() if c == ccnt)
        assert np.allclose(cm, _solve_linear(model, P, Q, draw_sample(SEED, hp, len(P), rc.S_OF[model])), rtol=1e-9, atol=1e-9)
    assert seen >= 14 and observable >= 5, (seen, observable)


def test_all_inlier_data_stop_at_the_first_valid_hypothesis(oracle):
    for name, model, P, Q, thr, expect in rc.cases():
        if name != "ties_all_inliers":
            continue
        first = next(h for h, m, err in _restated_hypotheses(model, P, Q, SEED))
        for conf in (0.5, 0.99):
            m, mask, cnt, used = oracle.estimate_ex(model, P, Q, thr, rc.RANSAC, confidence=conf, seed=SEED)
            assert cnt == len(P) and used == first + 1, (model, conf, used, first)
        m, mask, cnt, used = oracle.estimate_ex(model, P, Q, thr, rc.RANSAC, confidence=1.0, seed=SEED)
        assert used == K_HYP and cnt == len(P)


def test_tie_rule_lmeds_lowest_index_among_the_smallest_medians(oracle):
    seen = zero = denormal = observable = 0
    for name, model, P, Q, thr in _tie_cases(rc.LMEDS):
        n, s = len(P), rc.S_OF[model]
        hyp = [(h, m, np.sort(err)[n // 2]) for h, m, err in _restated_hypotheses(model, P, Q, SEED)]
        best = min(med for _, _, med in hyp)
        at_best = [(h, m) for h, m, med in hyp if med == best]
        assert len(at_best) >= 2 and np.isfinite(best), (name, model, best)
        hs, want = at_best[0]
        m, mask, cnt, used = oracle.estimate_ex(model, P, Q, thr, rc.LMEDS, seed=SEED)
        assert used == K_HYP and np.array_equal(m, want), (name, model, hs)
        others = [h for h, mo in at_best if not np.array_equal(mo, want)]  # (every LMedS tie class is an exact one)
        if name.startswith("ties_two_structures") or name in ("quantised_odd", "quantised_even", "quantised_denormal"):
            assert others, (name, model)
        if others:
            assert not np.array_equal(m, dict(at_best)[others[-1]]) and others[-1] > hs, (name, model, hs, others[-1])
            observable += 1
        err = restated_errors(model, want, P, Q)
        assert np.array_equal(mask.astype(bool), err <= _lmeds_thr2(err, thr, n, s)), (name, model)
        # rank n / 2 sits inside a run of equal keys
        run = int((err == best).sum())
        assert run >= 3, (name, model, run)
        assert name in EXACT, name
        zero += best == 0
        denormal += 0 < best < np.finfo(np.float64).tiny
        seen += 1
    assert seen >= 19 and zero >= 9 and denormal >= 2 and observable >= 10, (seen, zero, denormal, observable)


def test_large_sizes_are_past_65536_and_the_sampler_reaches_the_last_rows():
    for samp in (rc.RANSAC, rc.LMEDS):
        n = rc.LARGE_N[samp]
        top = max(max(draw_sample(SEED, h, n, 3)) for h in range(K_HYP))
        assert n > 65536 and top >= n - 100
