"""The pose-graph oracle (oracle/pg_oracle.c) on the census of tests/pg_adversarial_cases.py, against references that
are independent of it.  The kernels are held to the oracle in tests/test_pg_adversarial_gpu.py; where the two share a
formula only this file can find it wrong.

Residuals.  Every edge of every case: oracle.pg_edge_residual against an 80-digit mpmath evaluation of
log(M^-1 S_i^-1 S_j) -- the quaternion products in mpmath, the rotation vector as 2 atan(n / w) q / n, and the
translation part by solving W p = t with W = C I + A [r]x + B [r]x^2 from the branch-free closed forms of A, B, C (their
cancellation costs 36 of the 80 digits at theta = 1e-12 and is harmless), by mpmath.lu_solve, not by the oracle's
closed-form inverse.  Error = max over the components, relative to max(1, |t|) of the edge's composed transform.
Measured per class (test_edge_residuals_against_mpmath prints them); the bar of a class is 8 x its measured worst, and
no bar exceeds 1e-9:
    branch grid, theta = 0, 1e-12, 9.9e-6 (series branch)    2.3e-15   bar 1.9e-14
    branch grid, theta = 1.01e-5 (closed form, just above)   1.7e-12   bar 1.4e-11   <- (1 - cos theta) / theta^2 loses digits
    branch grid, theta = 1e-4                                 2.2e-13   bar 1.8e-12
    scales (frames 1e4 apart at scale 1e-3)                   3.0e-11   bar 2.4e-10   <- S_i^-1 S_j cancels 1e7 down to 32
    every other edge (theta from 0.05 to 3.1405, w < 0, ...)  7.1e-15   bar 5.7e-14
The loss just above theta = 1e-5 is a property of the pinned formulas (tests/golden/sim3_reference.npz holds them to
1e-12) and is recorded, not rewritten.  The loss in `scales` is the conditioning of the inputs: the relative
translation (t_j - t_i) / s_i is 1e7 in size and exact to 1e-9, the measurement takes all of it away but 32.

Solves.  Every case returns status 0; all_fixed and no_edges take 0 iterations with termination 2 and return the frames
bit for bit, as do the fixed and the edge-free frames of every other case; every other case lowers the cost.  For
both_ways, gps_gauge and dof_masks scipy.optimize.least_squares (its own finite differences, residuals through
scipy.linalg.logm of 4 x 4 matrices, the dof masks as missing parameters) reaches the oracle's final cost to 1e-6, the
bar of test_pose_graph_optimum_matches_scipy_least_squares."""
import os

import numpy as np
import pytest

import oracle_lib
import pg_adversarial_cases as pc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_reference.npz")
RESIDUAL_BAR = {"series": 8 * 2.3e-15, "above": 8 * 1.7e-12, "theta1e-4": 8 * 2.2e-13, "scales": 8 * 3.0e-11, "rest": 8 * 7.1e-15}
assert max(RESIDUAL_BAR.values()) <= 1e-9


def _opts(max_it=40):
    return oracle_lib.ba_options(max_iterations=max_it)


# ------------------------------------------------------------------------------------------------ mpmath reference
def _mp_residual(mp, etype, Si, Sj, meas):
    f = lambda v: mp.mpf(float(v))

    def qmul(a, b):
        return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def qrot(q, p):  # the oracle's formula, exact for a unit quaternion; the stored ones are unit to 1e-16 and the
        u = [2 * c for c in cross(q[:3], p)]  # oracle applies the same formula to the same numbers
        c2 = cross(q[:3], u)
        return [p[e] + q[3] * u[e] + c2[e] for e in range(3)]

    def mul(a, b):
        r = qrot(a[:4], [a[7] * b[4 + e] for e in range(3)])
        return qmul(a[:4], b[:4]) + [a[4 + e] + r[e] for e in range(3)] + [a[7] * b[7]]

    def inv(a):
        qc = [-a[0], -a[1], -a[2], a[3]]
        r = qrot(qc, a[4:7])
        return qc + [-r[e] / a[7] for e in range(3)] + [1 / a[7]]

    def lift(S, se3):
        S = [f(v) for v in S]
        return S[:7] + [mp.mpf(1) if se3 or len(S) == 7 else S[7]]

    se3 = etype != 1
    M, A = lift(meas, se3), lift(Si, se3)
    E = mul(inv(M), mul(inv(A), lift(Sj, se3))) if etype != 2 else mul(inv(M), A)
    n = mp.sqrt(E[0] ** 2 + E[1] ** 2 + E[2] ** 2)
    r = [mp.mpf(0)] * 3 if n == 0 else [E[e] / n * 2 * mp.atan(n / E[3]) for e in range(3)]
    th = mp.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)
    sg = mp.log(E[7])
    s = E[7]
    C = mp.mpf(1) if sg == 0 else (s - 1) / sg
    if th == 0 and sg == 0:
        A_, B_ = mp.mpf(1) / 2, mp.mpf(1) / 6
    elif th == 0:
        A_, B_ = ((sg - 1) * s + 1) / sg ** 2, ((sg ** 2 / 2 - sg + 1) * s - 1) / sg ** 3
    else:
        a, b, c = s * mp.sin(th), s * mp.cos(th), th ** 2 + sg ** 2
        A_ = (a * sg + (1 - b) * th) / (th * c)
        B_ = (C - ((b - 1) * sg + a * th) / c) / th ** 2
    K = mp.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    W = C * mp.eye(3) + A_ * K + B_ * (K * K)
    p = mp.lu_solve(W, mp.matrix(E[4:7]))
    out = [p[0], p[1], p[2]] + r + [sg]
    tnorm = mp.sqrt(E[4] ** 2 + E[5] ** 2 + E[6] ** 2)
    return np.array([float(v) for v in out[:6 if se3 else 7]]), float(tnorm), float(th)


def _graphs():
    for name in pc.NAMES:
        yield (name,) + pc.CASES[name]
    for name, g in pc.TWINS.items():
        yield (name + "_twin",) + g


def test_edge_residuals_against_mpmath(oracle):
    mp = pytest.importorskip("mpmath")
    worst = {}
    with mp.workdps(80):
        for name, start, dof, prob in _graphs():
            grid = name.startswith("branch_grid")
            edges = pc.all_edges(prob)
            total = 0.0
            for k, (t, i, j, m) in enumerate(edges):
                Sj = start[j] if j >= 0 else start[i]
                got = oracle.pg_edge_residual(t, start[i], Sj, m)
                ref, tnorm, th = _mp_residual(mp, t, start[i], Sj, m)
                err = float(np.abs(got - ref).max()) / max(1.0, tnorm)
                cls = "scales" if name == "scales" else "rest"
                if grid:
                    want = pc.ANGLES[k // len(pc.SIGMAS)]
                    assert abs(th - want) <= 1e-9 * want + 1e-15, (name, k, th, want)  # the case is on the side it names
                    assert abs(ref[6] - pc.SIGMAS[k % len(pc.SIGMAS)]) <= 4e-16, (name, k, ref[6])
                    cls = "series" if want < 1e-5 else "above" if want < 5e-5 else "theta1e-4"
                worst[cls] = max(worst.get(cls, 0.0), err)
                assert err <= RESIDUAL_BAR[cls], (name, k, t, err, th)
                total += 0.5 * float(ref @ ref)
            if name == "near_pi":
                ths = sorted(_mp_residual(mp, t, start[i], start[j], m)[2] for t, i, j, m in edges)[-4:]
                assert np.allclose(ths, [3.0, 3.0, 3.1405, 3.1405], atol=1e-9), ths
            if all(v[-1] is None for v in prob.values()):  # identity informations: the cost is the sum over the edges
                assert abs(oracle.pg_cost(start, prob) - total) <= 1e-12 * total, name
    print("worst residual error relative to max(1, |t|), per class:", dict((k, "%.1e" % v) for k, v in sorted(worst.items())))


def test_cost_is_the_sum_over_the_edges_with_informations(oracle):
    for name in ("info_mixed", "info_aniso", "info_zero_edge", "info_identity"):
        start, dof, prob = pc.CASES[name]
        total = 0.0
        for key, t, dim in (("se3", 0, 6), ("sim3", 1, 7), ("gps", 2, 6)):
            val = prob[key]
            for k in range(len(val[0])):
                i, j = int(val[0][k]), int(val[1][k]) if t != 2 else -1
                r = oracle.pg_edge_residual(t, start[i], start[j] if j >= 0 else start[i], val[-2][k])
                L = np.eye(dim) if val[-1] is None else val[-1][k].reshape(dim, dim)
                total += 0.5 * float(r @ L @ r)
        assert abs(oracle.pg_cost(start, prob) - total) <= 1e-12 * total, name


def test_sim3_algebra_stays_pinned_to_the_golden(oracle):
    g = np.load(GOLD)
    for i in range(len(g["mu"])):
        assert np.abs(oracle.sim3_exp(g["mu"][i]) - g["sims"][i]).max() < 1e-12
        assert np.abs(oracle.sim3_mul(g["sims"][i], g["sims"][(i + 1) % 64]) - g["muls"][i]).max() < 1e-12


@pytest.mark.parametrize("name", pc.NAMES)
def test_oracle_solves_the_census(oracle, name):
    start, dof, prob = pc.CASES[name]
    S, sm, st = oracle.pg_solve(start, dof, prob, _opts(), threads=4)
    assert st == 0
    for f in pc.fixed_frames(dof) + pc.UNTOUCHED.get(name, []):
        assert S[f].tobytes() == start[f].tobytes(), f
    print("%s: %d iterations (%d accepted), termination %d, cost %.6e -> %.6e" % (name, sm.iterations, sm.accepted, sm.termination,
                                                                                 sm.initial_cost, sm.final_cost))
    if name in pc.NOTHING_TO_DO:
        assert (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (0, 0, 2, 0) and S.tobytes() == start.tobytes()
        assert sm.final_cost == sm.initial_cost and (sm.initial_cost > 0) == (name == "all_fixed")
    else:
        assert sm.final_cost < sm.initial_cost and sm.accepted >= 1


def test_twins_are_the_same_problem(oracle):
    for name in ("neg_w", "info_identity"):
        a, b = pc.CASES[name], pc.TWINS[name]
        Sa, sa, _ = oracle.pg_solve(*a, _opts())
        Sb, sb, _ = oracle.pg_solve(*b, _opts())
        sign = -1.0 if name == "neg_w" else 1.0
        assert np.array_equal(Sa[:, :4], sign * Sb[:, :4]) and np.array_equal(Sa[:, 4:], Sb[:, 4:]), name
        assert list(sa.trace_cost[:sa.trace_len]) == list(sb.trace_cost[:sb.trace_len]) and sa.trace_len > 0
    a, b = pc.CASES["neg_w"], pc.TWINS["neg_w"]
    assert (a[0][:, 3] < 0).all() and all((v[-2][:, 3] < 0).all() for v in a[2].values()) and (b[0][:, 3] > 0).all()
    Sa, sa, _ = oracle.pg_solve(*pc.CASES["info_zero_edge"], _opts())
    Sb, sb, _ = oracle.pg_solve(*pc.TWINS["info_zero_edge"], _opts())
    assert sa.iterations == sb.iterations and np.abs(Sa - Sb).max() <= 1e-9 and abs(sa.final_cost - sb.final_cost) <= 1e-12 * sa.final_cost


def _mat(S):
    from scipy.spatial.transform import Rotation
    M = np.eye(4)
    M[:3, :3] = S[7] * Rotation.from_quat(S[:4]).as_matrix()
    M[:3, 3] = S[4:7]
    return M


@pytest.mark.parametrize("name", ["both_ways", "gps_gauge", "dof_masks"])
def test_optimum_matches_scipy_least_squares(oracle, name):
    from scipy.linalg import expm, logm
    from scipy.optimize import least_squares
    start, dof, prob = pc.CASES[name]
    S, sm, st = oracle.pg_solve(start, dof, prob, _opts(200))
    assert st == 0
    edges = pc.all_edges(prob)
    Minv = [np.linalg.inv(_mat(np.concatenate([m, [1.0]]) if len(m) == 7 else m)) for _, _, _, m in edges]
    M0 = [_mat(s) for s in S]  # from the oracle's optimum: an independent minimiser must not find a lower cost nearby ...
    Mstart = [_mat(s) for s in start]  # ... nor from the start
    slots = [(f, k) for f in range(len(start)) for k in range(7) if (dof[f] >> k) & 1]

    def hat(d):
        G = np.zeros((4, 4))
        G[:3, :3] = np.array([[d[6], -d[5], d[4]], [d[5], d[6], -d[3]], [-d[4], d[3], d[6]]])
        G[:3, 3] = d[:3]
        return G

    def unscale(Q):
        Q = Q.copy()
        Q[:3, :3] /= np.cbrt(np.linalg.det(Q[:3, :3]))
        return Q

    def make_fun(base):
        def fun(x):
            D = np.zeros((len(start), 7))
            for v, (f, k) in zip(x, slots):
                D[f, k] = v
            Ms = [base[f] @ expm(hat(D[f])) if D[f].any() else base[f] for f in range(len(start))]
            out = []
            for (t, i, j, m), Mi in zip(edges, Minv):
                A = Ms[i] if t == 1 else unscale(Ms[i])
                E = Mi @ A if t == 2 else Mi @ np.linalg.inv(A) @ (Ms[j] if t == 1 else unscale(Ms[j]))
                L = np.real(logm(E))
                out.append(np.array([L[0, 3], L[1, 3], L[2, 3], L[2, 1], L[0, 2], L[1, 0], L[0, 0]])[:7 if t == 1 else 6])
            return np.concatenate(out)
        return fun

    f0 = make_fun(M0)(np.zeros(len(slots)))
    assert abs(0.5 * float(f0 @ f0) - sm.final_cost) <= 1e-9 * sm.final_cost  # the same cost function, by another route
    res = least_squares(make_fun(Mstart), np.zeros(len(slots)), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12)
    print("%s: oracle %.9e  scipy %.9e" % (name, sm.final_cost, 0.5 * float(res.fun @ res.fun)))
    assert abs(0.5 * float(res.fun @ res.fun) - sm.final_cost) <= 1e-6 * sm.final_cost
