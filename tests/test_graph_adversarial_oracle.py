"""The general-graph oracle (oracle/graph_oracle.c) on the census of tests/graph_adversarial_cases.py, against references that
are independent of it.  The kernels are held to the oracle in tests/test_graph_adversarial_gpu.py; where the two share a
formula only this file can find it wrong.

Census.  From the inputs alone (numpy): observations per (landmark, frame) pair, the observation that carries a landmark's
host slot (hrep: the first valid one of a free inverse-depth point from another frame than its host), valid and invalid
observations at the start by the specification's depth / hemisphere rule, the counts against 16 / 64 / 128 / 256, the slots
of the busiest keyframe and the contributions to its diagonal block against the budget 2^K of the reproducible accumulation
(K = ceil(log2(4 x slots + landmarks / 64 + 16)), graph_det_budget) -- and every case is shown to reach what it is named
for (STRUCTURE below; a case without an entry fails the test).  The structural cases are also shown to MATTER: each solves
to another state than the graph it was cut from, by more than the bars of the GPU file.

Oracle runs.  Every case returns status 0 and lowers the cost, except the gate-only classes, of which only the gate is
asserted: everything_fixed / no_obs_nothing / behind_all / huber_1e-300 take 0 iterations with termination 2 and return the
state bit for bit.  nan_obs / inf_obs: initial cost NaN, three rejected iterations (a candidate cost of inf), termination
0, the state bit for bit.  nan_landmark / nan_frame: the observations of the poisoned block do not exist (a NaN depth fails
`> 1e-9`), the rest is solved, the NaN stays where it was and nowhere else.  step_pushes_behind: the first five candidates
cost `inf` and are rejected, and the dense step of this file puts the point at depth -0.01.  rho_floor: the three points end
at exactly 1e-9.  Fixed frames, fixed landmarks, landmarks without (valid) observations and fixed intrinsics come back bit
for bit everywhere.

Twins (test_twins): the same problem written differently solves to the same state, decision for decision.  Measured
largest difference after mapping back (frames and points absolute, inverse depths relative), bar = 8 x measured:
    obs_interleaved 4.5e-15   landmarks_relabelled 7.1e-15   frames_relabelled 5.3e-15   dup_is_double_info 7.1e-15
    behind_some 4.4e-15   unobserved_landmarks, first_nonhost_obs_invalid 2.2e-16 (the same float64 numbers)
The last three are twins of the base graph because what they add cannot reach it: landmarks nothing sees, observations
that do not exist.  frame_without_obs is no twin of its graph at this level: the extra edge changes the cost, hence the
radius of the later steps (the first six frames end 3.7e-10 apart).

Linearisation.  oracle_graph_obs / oracle_graph_obs_cam against a 50-digit mpmath evaluation of the specification:
Y = M(q_j)^T (X - t_j) or M(q_j)^T (s_h M(q_h) a + rho (t_h - t_j)) with M(q) = I + 2 w [v]x + 2 [v]x^2, the pinhole / OpenCV /
tangent-plane residual, and the Jacobians as central differences (h = 1e-20) along R <- R expm([w]x), t <- t + s R v,
s <- s exp(sigma), additive landmark and intrinsics, with mpmath's own matrix exponential; the Huber weight from its
definition; an observation exists on both sides or on neither.  Error = max |oracle - mpmath| / max(1, max |mpmath|) per
quantity (r, Jj, Jh, Jp, Jc, w).  Measured worst per class (test_linearisation_against_mpmath prints them); bar = 8 x
measured, never above 1e-9, and no figure is recorded below 2^-52:
    base (10 observations of the base graph)                                    2.2e-14   bar 1.8e-13
    depth_edge (depth 2e-9: Jacobians of 5e8; 1e-9 and 0.5e-9 do not exist)     2.2e-16   bar 1.8e-15   <- one ulp
    rho_edges (rho = 1e-7, 1e-9, 1e6; one of the latter behind its camera)      1.3e-15   bar 1.0e-14
    sim3_scales (keyframe scales 1e-3 and 1e3)                                  2.2e-15   bar 1.8e-14
    far_world (translations of 1e6)                                             7.1e-15   bar 5.7e-14
    info (rank-1, zero, 1e6 x, 1e-6 x informations, Huber on)                   2.8e-15   bar 2.2e-14
    huber_corner (s at h^2 and one ulp either side)                             2.2e-16   bar 1.8e-15   <- one ulp
    sphere (7 on the opposite hemisphere; bearings on axes and diagonals)       1.9e-15   bar 1.5e-14
    camera (beyond the fold of k1 = -0.28; within 0.02 of the centre)           6.7e-14   bar 5.4e-13
(far_world: X and t are 1e6 + a few metres, so X - t is exact in float64 and nothing of the offset is left in Y.)

First LM step.  The full Jacobian from the exported linearisation in numpy longdouble, the documented damping
clamp(diag, 1e-6, 1e32) / radius on every unknown, dof / free masks as removed columns, a dense elimination of the damped
normal equations (no Schur complement, no host slot, no landmark dimension), the oracle's exported retraction and the floor
of rho: the candidate's cost (oracle_graph_cost) against trace_cost[0].  Measured relative difference
(test_first_lm_step_without_schur prints it); bar = 8 x measured, at most 1e-9:
    all_frames_fixed 2.2e-16 (one ulp)   all_landmarks_fixed 3.0e-15   cam_underdetermined 2.0e-15 (radius 1, see below)
    dup_same_frame 4.9e-14   first_nonhost_obs_invalid 3.6e-14   hub_frame 8.6e-15   hub_landmark 6.1e-14
    lone_idp_host_only 9.5e-15   lone_idp_nonhost 4.8e-15   lone_xyz 2.4e-12 (rank-2 point blocks)   unobserved_landmarks 3.6e-14
cam_underdetermined is compared at an initial radius of 1 on both sides (gh_ba_options.initial_radius): six equations
for 33 coupled unknowns whose diagonals span 0.019 .. 6.9e5 leave, at the default radius of 1e4, a damped system of
condition ~1e12, and the float64 elimination of the oracle then differs from the longdouble one by 1.04e-9 in the
candidate's cost -- its own rounding, above the 1e-9 this file allows a bar.  At radius 1 the same algebra agrees to 2.0e-15.

Minimum.  huber_off and dup_is_double_info (well-posed, no robust kernel), solved to a function tolerance of 1e-14: the final
cost against scipy.optimize.least_squares on the same residuals with its own finite-difference Jacobians
(tests/test_graph_oracle._scipy_minimum).  Measured relative difference 4.2e-14 and 3.0e-14; bar 8 x that.

Yardstick.  Every finite case through oracle/liboracle.so and oracle/liboracle_fma.so (the same source with FMA
contraction): identical status, termination and accept / reject sequences, and the largest state difference and the largest
relative difference of a trace cost (beyond the 1e-15 absolute every comparison of costs here allows) per case within 2 x
of graph_adversarial_cases.YARDSTICK, which the GPU file takes its bars from.  Measured (test_yardstick prints every case):
    state: 1e-15 .. 3e-14 on the graphs cut from the base graph, the landmark boundaries and the camera cases with 127 and more
           observations; one_frame 1.8e-13, lone_xyz 4.7e-13, rho_huge 7.1e-13 (rank-2 or stiff point blocks);
           sim3_scales 1.3e-12; cam_unobservable 2.1e-12; tangent_axis_ties 6.7e-12; frame_without_obs 1.4e-11 and
           no_obs_pose_edges 9.3e-12 (pose edges: finite-difference Jacobians); obs_15 / 16 / 17 1e-12 .. 8e-12 and
           cam_obs_63 / 64 / 65 7e-12 .. 1.1e-11 (the cut leaves many landmarks one observation); info_rank1_zero_scales
           4.3e-10 and cam_underdetermined 1.2e-9 (three iterations each)
    cost:  0 (below the 1e-15 absolute) on most; up to 1e-11 elsewhere except frame_without_obs 9.2e-11, obs_15 / 16 / 17
           9e-11 .. 7e-10, cam_obs_63 / 64 / 65 5e-10 .. 8e-10, no_obs_pose_edges 2.6e-9, cam_underdetermined 6.6e-9
"""
import os

import numpy as np
import pytest

import graph_adversarial_cases as gc
import oracle_lib

ULP = 2.0 ** -52  # the resolution of every measured figure: the relative difference of two float64 numbers
LIN_BAR = {"base": 8 * 2.2e-14, "depth_edge": 8 * ULP, "rho_edges": 8 * 1.3e-15, "sim3_scales": 8 * 2.2e-15, "far_world": 8 * 7.1e-15,
           "info": 8 * 2.8e-15, "huber_corner": 8 * ULP, "sphere": 8 * 1.9e-15, "camera": 8 * 6.7e-14}
STEP_BAR = {"all_frames_fixed": 8 * ULP, "all_landmarks_fixed": 8 * 3.0e-15, "cam_underdetermined": 8 * 2.0e-15, "dup_same_frame": 8 * 4.9e-14,
            "first_nonhost_obs_invalid": 8 * 3.6e-14, "hub_frame": 8 * 8.6e-15, "hub_landmark": 8 * 6.1e-14, "lone_idp_host_only": 8 * 9.5e-15,
            "lone_idp_nonhost": 8 * 4.8e-15, "lone_xyz": 8 * 2.4e-12, "unobserved_landmarks": 8 * 3.6e-14}
TWIN_BAR = {"obs_interleaved": 8 * 4.5e-15, "landmarks_relabelled": 8 * 7.1e-15, "frames_relabelled": 8 * 5.3e-15, "dup_is_double_info": 8 * 7.1e-15,
            "unobserved_landmarks": 8 * ULP, "first_nonhost_obs_invalid": 8 * ULP, "behind_some": 8 * 4.4e-15}
MIN_BAR = {"huber_off": 8 * 4.2e-14, "dup_is_double_info": 8 * 3.0e-14}
assert max(list(LIN_BAR.values()) + list(STEP_BAR.values()) + list(TWIN_BAR.values()) + list(MIN_BAR.values())) <= 1e-9
STEP_RADIUS = {"cam_underdetermined": 1.0}  # see the module docstring
MATTERS = 1e-7  # the widest state bar of the GPU file: a feature that moves the solution by less would not be seen there


def solve(orc, case, max_iterations=None, function_tolerance=None, initial_radius=None):
    """-> {"S", "xyz", "rho", "cam" (None without intrinsics), "sm", "st"}"""
    opts = oracle_lib.ba_options(huber=case["huber"], max_iterations=case["max_iterations"] if max_iterations is None else max_iterations)
    if function_tolerance is not None:
        opts.function_tolerance = function_tolerance
    if initial_radius is not None:
        opts.initial_radius = initial_radius
    if case["problem"].get("intrinsics") is not None:
        S, xyz, rho, cam, sm, st = orc.graph_solve_cam(case["start"], case["dof"], case["problem"], opts)
    else:
        (S, xyz, rho, sm, st), cam = orc.graph_solve(case["start"], case["dof"], case["problem"], opts), None
    return {"S": S, "xyz": xyz, "rho": rho, "cam": cam, "sm": sm, "st": st}


def accepts(sm):
    return [int(sm.trace_accepted[i]) for i in range(sm.trace_len)]


def costs(sm):
    return [sm.trace_cost[i] for i in range(sm.trace_len)]


def state_difference(a, b, twin=None):
    """Frames and points absolute, inverse depths relative, focal lengths / principal point relative, distortion absolute.
    twin: index arrays that put a's blocks into b's order."""
    twin = twin or {}
    pick = lambda arr, key: arr if twin.get(key) is None else arr[twin[key]]
    d = [ULP * 0.0]
    for key, name, rel in (("frames", "S", False), ("xyz", "xyz", False), ("idp", "rho", True)):
        x, y = pick(a[name], key), b[name]
        if y.size:
            d.append(float(np.nanmax(np.abs(x - y) / (np.abs(y) if rel else 1.0))))
    if b["cam"] is not None:
        d.append(float(np.max(np.abs(a["cam"][:4] - b["cam"][:4]) / np.abs(b["cam"][:4]))))
        d.append(float(np.max(np.abs(a["cam"][4:] - b["cam"][4:]))))
    return max(d)


def cost_difference(sa, sb):
    """The smallest rtol at which |a - b| <= 1e-15 + rtol |b| holds over the initial cost, the trace and the final cost."""
    worst = 0.0
    for x, y in zip([sa.initial_cost, sa.final_cost] + costs(sa), [sb.initial_cost, sb.final_cost] + costs(sb)):
        if np.isfinite(y) and y != 0.0:
            worst = max(worst, max(abs(x - y) - 1e-15, 0.0) / abs(y))
    return worst


# ------------------------------------------------------------------------------------------------ census
def census(case):
    pr = case["problem"]
    kind, point, frame = pr["obs"][:3]
    nf, nx, ni, no = len(case["dof"]), len(pr["xyz"][0]), len(pr["idp"][2]), len(kind)
    lm, host = gc.obs_landmark(pr), gc.obs_host(pr)
    valid = gc.valid_at_start(case)
    M = np.zeros((nx + ni, nf), np.int64)
    np.add.at(M, (lm, frame), 1)
    free = np.concatenate([np.asarray(pr["xyz"][1]) != 0, np.asarray(pr["idp"][3]) != 0])
    hrep = np.full(ni, -1)
    for k in range(no - 1, -1, -1):
        if kind[k] == 1 and valid[k] and frame[k] != host[k] and free[nx + point[k]]:
            hrep[point[k]] = k
    slots = np.bincount(frame, minlength=nf) + np.bincount(host[(kind == 1) & (host != frame)], minlength=nf)
    most = 4 * max(16, int(slots.max()) if no else 0) + (nx + ni) // 64 + 16
    # contributions to one word of a keyframe's diagonal block: one per slot in gr_frame_rows; in gr_schur one per ordered pair
    # of a landmark's slots in that keyframe (the host slots of a landmark are one)
    per_lm_frame = M.copy()
    for p in range(ni):
        if hrep[p] >= 0:
            per_lm_frame[nx + p, pr["idp"][0][p]] += 1
    diag_words = int(max(slots.max() if no else 0, (per_lm_frame ** 2).sum(axis=0).max() if no else 0))
    return {"nf": nf, "nx": nx, "ni": ni, "no": no, "M": M, "per_lm": M.sum(axis=1), "per_frame": np.bincount(frame, minlength=nf), "valid": valid,
            "hrep": hrep, "slots": slots, "K": int(np.ceil(np.log2(most))), "diag_words": diag_words, "waves": 2 * -(-max(no, 1) // 128),
            "kind": kind, "point": point, "frame": frame, "host": host, "lm": lm}


def _shuffled(c, case):
    b = gc.CASES["base"]["problem"]["obs"]
    runs = 1 + int((np.diff(c["kind"]) != 0).sum())
    return (runs > 40 and sorted(zip(c["kind"], c["point"], c["frame"])) == sorted(zip(*b[:3])) and not np.array_equal(c["lm"], np.sort(c["lm"]))
            and np.array_equal(np.sort(b[2]), np.sort(c["frame"])))


def _relabelled(key):
    def check(c, case):
        perm = gc.TWINS["%s_relabelled" % key][{"landmarks": "xyz", "frames": "frames"}[key]]
        b = gc.CASES["base"]
        if key == "frames":
            return (perm[0] != 0 and case["dof"][perm[0]] == 0 and np.array_equal(case["start"][perm], b["start"]) and np.array_equal(case["dof"][perm], b["dof"])
                    and np.array_equal(perm[b["problem"]["obs"][2]], c["frame"]) and (perm[b["problem"]["idp"][0]] != b["problem"]["idp"][0]).any())
        pi = gc.TWINS["landmarks_relabelled"]["idp"]
        return (not np.array_equal(perm, np.arange(len(perm))) and np.array_equal(case["problem"]["xyz"][0][perm], b["problem"]["xyz"][0])
                and np.array_equal(case["problem"]["idp"][2][pi], b["problem"]["idp"][2]) and np.array_equal(case["problem"]["idp"][0][pi], b["problem"]["idp"][0]))
    return check


def _dup_same_frame(c, case):
    M, nx = c["M"], c["nx"]
    h1 = case["problem"]["idp"][0][1]
    return (M[0].max() == gc.DUP and M[nx].max() == gc.DUP and M[nx, case["problem"]["idp"][0][0]] == 1 and M[nx + 1, h1] == 3
            and c["diag_words"] >= gc.DUP ** 2 and M[np.arange(len(M)) > 0][:, :].max() <= gc.DUP and (M[1:nx] <= 1).all())


def _lone(which):
    def check(c, case):
        nx, kind, host, frame = c["nx"], c["kind"], c["host"], c["frame"]
        rows = range(gc.LONE) if which == "xyz" else range(nx, nx + gc.LONE)
        if not all(c["per_lm"][p] == 1 for p in rows) or (np.delete(c["per_lm"], list(rows)) < 3).any():
            return False
        ks = [int(np.flatnonzero(c["lm"] == p)[0]) for p in rows]
        if which == "xyz":
            return all(kind[k] == 0 for k in ks)
        own = [frame[k] == host[k] for k in ks]
        return all(own) and (c["hrep"][:gc.LONE] == -1).all() if which == "idp_host_only" else not any(own) and list(c["hrep"][:gc.LONE]) == ks
    return check


def _unobserved(c, case):
    nx, ni = c["nx"], c["ni"]
    want_x, want_i = [0, 1, nx // 2 - 1, nx // 2, nx - 2, nx - 1], [0, 1, ni // 2 - 1, ni // 2, ni - 2, ni - 1]
    none = np.flatnonzero(c["per_lm"] == 0)
    xfree, ifree = case["problem"]["xyz"][1], case["problem"]["idp"][3]
    return (list(none) == want_x + [nx + p for p in want_i] and list(xfree[want_x]) == [1, 0] * 3 and list(ifree[want_i]) == [1, 0] * 3
            and nx == 26 and ni == 26)


def _frame_without_obs(c, case):
    first, second = case["problem"]["se3"][:2]
    touched = np.bincount(np.concatenate([first, second]), minlength=c["nf"])
    return (c["nf"] == 8 and list(c["per_frame"][6:]) == [0, 0] and list(c["slots"][6:]) == [0, 0] and touched[6] == 0 and touched[7] == 1
            and list(case["dof"][6:]) == [63, 63] and c["per_frame"][:6].min() > 0)


def _host_groups(hosts_fixed):
    def check(c, case):
        A = np.isin(np.arange(8), gc.GROUP_A)
        idp = c["kind"] == 1
        seen = sorted(set(c["point"][idp]))
        hosts = case["problem"]["idp"][0][seen]
        observers = c["frame"][idp & (c["frame"] != c["host"])]
        return (len(seen) >= 5 and (A[hosts] == hosts_fixed).all() and (A[observers] != hosts_fixed).all() and len(observers) >= 2 * len(seen)
                and list(case["dof"]) == [0] * 4 + [63] * 4 and (c["hrep"][seen] >= 0).all())
    return check


def _one_host(hub):
    def check(c, case):
        ok = (case["problem"]["idp"][0] == 3).all() and case["dof"][3] == 63 and c["slots"][3] >= c["ni"]
        sees_all = (c["M"][:, 3] >= 1).all()
        return ok and (sees_all and c["slots"][3] == c["slots"].max() and c["per_frame"][3] == c["nx"] + c["ni"] if hub else not sees_all)
    return check


def _first_invalid(c, case):
    ks = list(range(gc.LONE))
    return (list(c["point"][ks]) == ks and (c["kind"][ks] == 1).all() and (c["frame"][ks] == 6).all() and not c["valid"][ks].any() and c["valid"][gc.LONE:].all()
            and all(gc.obs_Y(case, k)[2] < -0.1 for k in ks) and all(c["hrep"][p] > gc.LONE and c["frame"][c["hrep"][p]] != c["host"][c["hrep"][p]] for p in ks)
            and all(int(np.flatnonzero((c["lm"] == c["nx"] + p) & (c["frame"] != c["host"]))[0]) == p for p in ks))


def _behind_some(c, case):
    bad = ~c["valid"]
    return (bad.sum() == 2 * gc.BEHIND and (c["frame"][bad] == 6).all() and (c["frame"][~bad] != 6).all() and sorted(c["kind"][bad]) == [0] * gc.BEHIND + [1] * gc.BEHIND
            and all(gc.obs_Y(case, k)[2] < -0.1 for k in np.flatnonzero(bad)) and np.flatnonzero(bad).max() - np.flatnonzero(bad).min() > 40)


def _hub_landmark(c, case):
    return (c["nf"] == 12 and (c["M"][0] == 1).all() and (c["M"][c["nx"]] == 1).all() and c["per_lm"][0] == 12 and c["per_lm"][c["nx"]] == 12
            and np.delete(c["per_lm"], [0, c["nx"]]).max() == 4)


def _few_frames(n):
    def check(c, case):
        own = c["frame"] == c["host"]
        return (c["nf"] == n and case["dof"][0] == 0 and (n == 1 or case["dof"][1] == 62) and c["no"] > 0 and (n > 1 or own[c["kind"] == 1].all())
                and (case["problem"]["idp"][0] < n).all())
    return check


def _lm_edge(n):
    return lambda c, case: c["nx"] + c["ni"] == n and -(-n // 256) == (1 if n <= 256 else 2) and c["per_lm"].min() == 3 and c["ni"] > 0 and c["nx"] > 0


def _obs_edge(n):
    return lambda c, case: (c["no"] == n and case["problem"].get("intrinsics") is None and -(-16 * n // 256) == (1 if n <= 16 else 2)
                            and (c["kind"] == 0).any() and (c["kind"] == 1).any() and (c["frame"] != c["host"])[c["kind"] == 1].any())


def _cam_obs_edge(n):
    def check(c, case):
        cam, free = case["problem"]["intrinsics"]
        return (c["no"] == n and free == 15 and c["waves"] == 2 * -(-n // 128) and -(-n // 64) == {1: 1, 63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3}[n]
                and -(-16 * n // 256) == -(-n // 16) and c["valid"].all())
    return check


def _depth_edge(c, case):
    ks = [c["no"] - 3, c["no"] - 2, c["no"] - 1]
    z = [gc.obs_Y(case, k)[2] for k in ks]
    pts = case["problem"]["xyz"][0][-3:]
    return (z == [0.5e-9, 1e-9, 2e-9] and all(gc.obs_Y(case, k).tobytes() == pts[i].tobytes() for i, k in enumerate(ks)) and list(c["valid"][ks]) == [False, False, True]
            and c["valid"][:-3].all() and list(c["per_lm"][c["nx"] - 3:c["nx"]]) == [1, 1, 1] and case["dof"][6] == 0)


def _step_pushes_behind(c, case):
    Y = gc.obs_Y(case, c["no"] - 1)
    return c["valid"].all() and Y.tobytes() == np.array([0.01, 0.0, 0.01]).tobytes() and case["huber"] == 0.0 and c["per_lm"][c["nx"] - 1] == 1


def _rho_floor(c, case):
    rho = case["problem"]["idp"][2]
    return (rho[:gc.RHO_FLOOR_POINTS] == 1e-7).all() and rho[gc.RHO_FLOOR_POINTS:].min() > 0.05 and c["valid"].all() and (c["hrep"][:gc.RHO_FLOOR_POINTS] >= 0).all()


def _info_sorts(c, case):
    L = case["problem"]["obs"][4].reshape(-1, 2, 2)
    b = gc.graph(with_info=True)["problem"]["obs"][4].reshape(-1, 2, 2)
    ev, s = np.linalg.eigvalsh(L), gc.INFO_SORT
    return (np.array_equal(L, L.transpose(0, 2, 1)) and all((s == k).sum() >= 8 for k in range(4)) and (np.abs(ev[s == 0, 0]) <= 1e-15 * ev[s == 0, 1]).all()
            and not L[s == 1].any() and np.array_equal(L[s == 2], 1e6 * b[s == 2]) and np.array_equal(L[s == 3], 1e-6 * b[s == 3])
            and np.array_equal(L[s > 3], b[s > 3]) and (ev[s > 0, 0] >= 0).all() and case["max_iterations"] == 3)


def _huber_corner(c, case):
    h, xy = gc.HUBER_CORNER, case["problem"]["obs"][3][-3:]
    s = [float(m[0]) * float(m[0]) + float(m[1]) * float(m[1]) for m in xy]
    return (case["huber"] == h and all(gc.obs_Y(case, k).tobytes() == np.array([0.0, 0.0, 2.0]).tobytes() for k in range(c["no"] - 3, c["no"]))
            and [v > h * h for v in s] == [False, False, True] and s[1] == h * h and s[0] < s[1] and xy[0, 0] == -np.nextafter(h, 0))


def _sim3_scales(c, case):
    s = case["start"][:, 7]
    b = gc.graph(kind="sim3")
    return (list(case["dof"]) == [0, 126, 127, 127, 127, 127] and 5e-4 < s[2] < 2e-3 and 5e2 < s[4] < 2e3 and (np.delete(s, [2, 4]) > 0.8).all() and (np.delete(s, [2, 4]) < 1.25).all()
            and (case["problem"]["idp"][0] == 2).any() and (case["problem"]["idp"][0] == 4).any() and c["valid"].all()
            and np.allclose([gc.obs_Y(case, k)[:2] / gc.obs_Y(case, k)[2] for k in range(c["no"])],
                            [gc.obs_Y(gc._case(b), k)[:2] / gc.obs_Y(gc._case(b), k)[2] for k in range(c["no"])], rtol=1e-9, atol=1e-12))


def _far_world(c, case):
    return (np.abs(case["start"][:, 4:7]).min() > 9.9e5 and np.abs(case["problem"]["xyz"][0]).min() > 9.9e5 and c["valid"].all()
            and max(np.abs(gc.obs_Y(case, k)).max() for k in range(c["no"])) < 30.0)


def _opposite(c, case):
    bad = ~c["valid"]
    return case["problem"]["projection"] == "sphere" and bad.sum() == 20 and list(np.flatnonzero(bad)) == list(range(0, 160, 8)) and sorted(set(c["kind"][bad])) == [0, 1]


def _axis(b):
    """The specification's rule in words: the axis b is least aligned with; ties go to x, then y."""
    a = np.abs(b)
    return min(range(3), key=lambda i: (a[i], i))


def _tangent_ties(c, case):
    b = case["problem"]["obs"][3][-len(gc.AXES):]
    chosen = [_axis(v) for v in b]
    ties = [sorted(np.abs(v))[0] == sorted(np.abs(v))[1] for v in b]
    all_equal = [np.abs(v).min() == np.abs(v).max() for v in b]
    return (c["valid"].all() and set(chosen) == {0, 1, 2} and sum(ties) >= 9 and sum(all_equal) == 3 and chosen[:3] == [1, 0, 0] and chosen[6:9] == [2, 1, 0]
            and all(chosen[i] == 0 for i in range(12, 15)) and chosen[15:] == [0, 1, 2] and np.allclose(np.linalg.norm(b, axis=1), 1.0, atol=2e-16))


def _normalised(case):
    return np.array([gc.obs_Y(case, k)[:2] / gc.obs_Y(case, k)[2] for k in range(len(case["problem"]["obs"][0]))])


def _cam(free, extra=lambda c, case: True):
    return lambda c, case: case["problem"]["intrinsics"][1] == free and c["valid"].all() and case["problem"]["intrinsics"][0][0] != 0 and extra(c, case)


def _poison(where):
    def check(c, case):
        blocks = {"obs": case["problem"]["obs"][3], "xyz": case["problem"]["xyz"][0], "frames": case["start"], "rho": case["problem"]["idp"][2]}
        return (all((~np.isfinite(v)).sum() == (1 if k == where else 0) for k, v in blocks.items()) and case["max_iterations"] <= 3
                and (where != "frames" or np.isfinite(case["start"][:, 7]).all()))
    return check


_base = lambda c, case: c["valid"].all() and (c["M"] <= 1).all() and c["per_lm"].min() == 4 and c["per_frame"].min() > 0 and (c["hrep"] >= 0).all()
STRUCTURE = {
    "base": lambda c, case: _base(c, case) and np.array_equal(c["lm"], np.sort(c["lm"])),
    "obs_interleaved": _shuffled, "landmarks_relabelled": _relabelled("landmarks"), "frames_relabelled": _relabelled("frames"),
    "dup_same_frame": _dup_same_frame,
    "dup_is_double_info": lambda c, case: (c["M"] == 2 * census(gc.CASES["double_info"])["M"]).all() and case["huber"] == 0.0 and case["problem"]["obs"][4] is None,
    "double_info": lambda c, case: _base(c, case) and np.array_equal(case["problem"]["obs"][4], np.tile([2.0, 0, 0, 2.0], (c["no"], 1))) and case["huber"] == 0.0,
    "lone_xyz": _lone("xyz"), "lone_idp_nonhost": _lone("idp_nonhost"), "lone_idp_host_only": _lone("idp_host_only"),
    "unobserved_landmarks": _unobserved, "frame_without_obs": _frame_without_obs,
    "all_landmarks_fixed": lambda c, case: not case["problem"]["xyz"][1].any() and not case["problem"]["idp"][3].any() and (case["dof"][1:] != 0).all() and (c["hrep"] == -1).all(),
    "all_frames_fixed": lambda c, case: not case["dof"].any() and case["problem"]["xyz"][1].all() and case["problem"]["idp"][3].all(),
    "everything_fixed": lambda c, case: not case["dof"].any() and not case["problem"]["xyz"][1].any() and not case["problem"]["idp"][3].any() and c["no"] == 160,
    "no_obs_pose_edges": lambda c, case: c["no"] == 0 and c["nx"] == 20 and c["ni"] == 20 and len(case["problem"]["se3"][0]) >= 6,
    "no_obs_nothing": lambda c, case: c["no"] == 0 and c["nx"] == 20 and c["ni"] == 20 and not any(k in case["problem"] for k in ("se3", "sim3", "gps")),
    "hosts_fixed_observers_free": _host_groups(True), "hosts_free_observers_fixed": _host_groups(False),
    "one_host_for_all": _one_host(False), "hub_frame": _one_host(True), "first_nonhost_obs_invalid": _first_invalid, "hub_landmark": _hub_landmark,
    "one_frame": _few_frames(1), "two_frames": _few_frames(2),
    "cam_waves_18": lambda c, case: c["no"] == 1100 and c["waves"] == 18 and c["waves"] % 16 == 2 and case["problem"]["intrinsics"][1] == 31 and c["nx"] + c["ni"] == 275,
    "info_rank1_zero_scales": _info_sorts, "depth_edge": _depth_edge, "behind_some": _behind_some,
    "behind_all": lambda c, case: not c["valid"].any() and c["no"] == 160 and c["ni"] == 0 and all(gc.obs_Y(case, k)[2] < -1.0 for k in range(160)),
    "step_pushes_behind": _step_pushes_behind, "rho_floor": _rho_floor,
    "rho_huge": lambda c, case: (case["problem"]["idp"][2][:3] == 1e6).all() and (~c["valid"]).sum() == 3 and c["valid"][(c["kind"] == 1) & (c["point"] < 3)].sum() >= 6,
    "huber_off": lambda c, case: case["huber"] == 0.0, "huber_1e300": lambda c, case: case["huber"] == 1e300, "huber_1e-300": lambda c, case: case["huber"] == 1e-300,
    "huber_corner": _huber_corner, "sim3_scales": _sim3_scales, "far_world": _far_world, "opposite_hemisphere": _opposite, "tangent_axis_ties": _tangent_ties,
    "cam_fixed_pixels": _cam(0, lambda c, case: np.array_equal(case["problem"]["intrinsics"][0], gc.CAM)),
    "cam_unobservable": _cam(0b111000000, lambda c, case: np.abs(_normalised(case)).max() < 0.02 and c["ni"] == 0),
    "cam_underdetermined": _cam(0x1FF, lambda c, case: c["no"] == 3),
    "cam_fold_over": _cam(31, lambda c, case: (np.linalg.norm(_normalised(case), axis=1) > gc.FOLD_RADIUS).sum() >= 5 and case["problem"]["intrinsics"][0][4] == -0.28 + 0.02 and gc.CAM_K1[4] == -0.28
                          and not case["problem"]["intrinsics"][0][5:].any()),
    "nan_obs": _poison("obs"), "inf_obs": _poison("obs"), "nan_landmark": _poison("xyz"), "nan_frame": _poison("frames")}
STRUCTURE.update(("lm_%d" % n, _lm_edge(n)) for n in gc.LM_EDGES)
STRUCTURE.update(("obs_%d" % n, _obs_edge(n)) for n in gc.OBS_EDGES)
STRUCTURE.update(("cam_obs_%d" % n, _cam_obs_edge(n)) for n in gc.CAM_OBS_EDGES)


def test_every_case_reaches_what_it_is_named_for():
    assert sorted(STRUCTURE) == sorted(gc.NAMES)
    seen = {}
    for name in gc.NAMES:
        case = gc.CASES[name]
        c = census(case)
        seen[name] = c
        print("%-28s frames %2d xyz %3d idp %3d obs %4d (invalid %3d)  obs / (landmark, frame) max %2d  slots of the busiest frame %3d, K %d, diagonal words %4d  waves %2d" % (
            name, c["nf"], c["nx"], c["ni"], c["no"], (~c["valid"]).sum(), c["M"].max() if c["no"] else 0, c["slots"].max(), c["K"], c["diag_words"], c["waves"]))
        assert STRUCTURE[name](c, case), name
        assert c["nf"] <= 12 and c["nx"] + c["ni"] <= 300 and case["max_iterations"] <= 40
        # the reproducible accumulation: every word gets fewer contributions than its budget 2^K, the m^2 of dup_same_frame included
        assert c["diag_words"] + c["waves"] < 2 ** c["K"], name
    # what the census as a whole must contain
    assert {255, 256, 257} <= set(c["nx"] + c["ni"] for c in seen.values())
    assert set(gc.OBS_EDGES) | set(gc.CAM_OBS_EDGES) | {1100} <= set(c["no"] for c in seen.values())
    assert seen["dup_same_frame"]["diag_words"] >= 144 > seen["dup_same_frame"]["slots"].max()  # m^2 contributions against "usually 1"
    assert seen["hub_frame"]["slots"].max() > 2 * seen["one_host_for_all"]["per_frame"].max()
    assert sorted(gc.TWINS) == sorted(TWIN_BAR) and set(gc.MAX_IT) <= set(gc.NAMES)


# ------------------------------------------------------------------------------------------------ oracle runs
@pytest.fixture(scope="module")
def runs(oracle):
    return dict((name, solve(oracle, gc.CASES[name])) for name in gc.NAMES)


def same_state(got, case):
    pr = case["problem"]
    return (got["S"].tobytes() == case["start"].tobytes() and got["xyz"].tobytes() == np.ascontiguousarray(pr["xyz"][0], np.float64).tobytes()
            and got["rho"].tobytes() == np.ascontiguousarray(pr["idp"][2], np.float64).tobytes()
            and (got["cam"] is None or got["cam"].tobytes() == np.ascontiguousarray(pr["intrinsics"][0], np.float64).tobytes()))


def untouched(got, case, name):
    """The blocks the case marks come back bit for bit; whatever was finite going in is finite coming out."""
    pr = case["problem"]
    for f in gc.fixed_frames(case):
        assert got["S"][f].tobytes() == case["start"][f].tobytes(), (name, "fixed frame", f)
    for p in gc.still_xyz(case):
        assert got["xyz"][p].tobytes() == np.asarray(pr["xyz"][0][p], np.float64).tobytes(), (name, "XYZ point", p)
    for p in gc.still_idp(case):
        assert got["rho"][p] == pr["idp"][2][p], (name, "inverse-depth point", p)
    for k in gc.fixed_intrinsics(case):
        assert got["cam"][k] == pr["intrinsics"][0][k], (name, "intrinsic", k)
    assert np.isfinite(got["S"][np.isfinite(case["start"])]).all() and np.isfinite(got["xyz"][np.isfinite(pr["xyz"][0])]).all() and np.isfinite(got["rho"]).all(), name
    assert (got["rho"] >= gc.RHO_FLOOR).all() and (got["S"][:, 7] > 0).all(), name


@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_on_the_census(runs, name):
    case, got = gc.CASES[name], runs[name]
    sm, st = got["sm"], got["st"]
    print("%s: status %d, %d iterations (%d accepted), termination %d, cost %.6e -> %.6e, decisions %s" % (
        name, st, sm.iterations, sm.accepted, sm.termination, sm.initial_cost, sm.final_cost, "".join(str(a) for a in accepts(sm))))
    assert st == 0
    untouched(got, case, name)
    if name in gc.NOTHING_TO_DO:
        assert (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (0, 0, 2, 0) and same_state(got, case) and sm.final_cost == sm.initial_cost
    elif name in ("nan_obs", "inf_obs"):
        assert (sm.iterations, sm.accepted, sm.termination, sm.trace_len) == (3, 0, 0, 3) and np.isnan(sm.initial_cost) and np.isnan(sm.final_cost)
        assert all(v == np.inf for v in costs(sm)) and same_state(got, case)
    else:
        assert sm.final_cost < sm.initial_cost and sm.accepted >= 1 and np.isfinite(sm.initial_cost) and sm.trace_len == sm.iterations
        if name == "nan_landmark":
            assert np.isnan(got["xyz"][3, 0]) and got["xyz"][3, 1:].tobytes() == case["problem"]["xyz"][0][3, 1:].tobytes()
        elif name == "nan_frame":
            assert np.isnan(got["S"][2]).any() and np.isfinite(np.delete(got["S"], 2, axis=0)).all()
        else:
            assert np.isfinite(got["S"]).all() and (got["cam"] is None or np.isfinite(got["cam"]).all())
    if name == "depth_edge":  # at and below 1e-9 the observation does not exist; the third point moves
        assert got["xyz"][-1].tobytes() != case["problem"]["xyz"][0][-1].tobytes()
    if name == "step_pushes_behind":
        assert accepts(sm)[:6] == [0, 0, 0, 0, 0, 1] and all(v == np.inf for v in costs(sm)[:5]) and np.isfinite(costs(sm)[5:]).all()
    if name == "rho_floor":
        assert (got["rho"][:gc.RHO_FLOOR_POINTS] == gc.RHO_FLOOR).all() and 0 in accepts(sm) and got["rho"][gc.RHO_FLOOR_POINTS:].min() > 0.05
    if name == "lone_idp_host_only":
        assert gc.still_idp(case) == list(range(gc.LONE))
    if name in ("all_landmarks_fixed", "all_frames_fixed"):
        assert (got["S"].tobytes() == case["start"].tobytes()) == (name == "all_frames_fixed")
        assert (got["xyz"].tobytes() == case["problem"]["xyz"][0].tobytes() and got["rho"].tobytes() == case["problem"]["idp"][2].tobytes()) == (name == "all_landmarks_fixed")
    if name == "cam_fixed_pixels":
        assert got["cam"].tobytes() == gc.CAM.tobytes()


def test_gate_classes_agree_with_their_twins(runs):
    """Huber off and huge are the same problem, bit for bit."""
    a, b = runs["huber_off"], runs["huber_1e300"]
    assert a["S"].tobytes() == b["S"].tobytes() and a["xyz"].tobytes() == b["xyz"].tobytes() and a["rho"].tobytes() == b["rho"].tobytes()
    assert costs(a["sm"]) == costs(b["sm"])


@pytest.mark.parametrize("name", sorted(gc.TWINS))
def test_twins(runs, name):
    twin = gc.TWINS[name]
    a, b = runs[name], runs[twin["of"]]
    assert accepts(a["sm"]) == accepts(b["sm"]) and a["sm"].termination == b["sm"].termination
    d = max(state_difference(a, b, twin), ULP)
    c = cost_difference(a["sm"], b["sm"])
    print("%s against %s: state %.1e, costs %.1e (bar %.1e)" % (name, twin["of"], d, c, TWIN_BAR[name]))
    assert d <= TWIN_BAR[name] and c <= 1e-12


def test_structural_features_matter(oracle, runs):
    for name, plain in gc.featureless().items():
        a, b = runs[name], solve(oracle, plain)
        nf, nx = min(len(a["S"]), len(b["S"])), min(len(a["xyz"]), len(b["xyz"]))
        d = max(float(np.abs(a["S"][:nf] - b["S"][:nf]).max()), float(np.abs(a["xyz"][:nx] - b["xyz"][:nx]).max()))
        print("%s: differs from the graph without the feature by %.1e" % (name, d))
        assert d > MATTERS, name


# ------------------------------------------------------------------------------------------------ linearisation
def _mp_rot(mp, q):
    x, y, z, w = q
    K = mp.matrix([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return mp.eye(3) + 2 * w * K + 2 * (K * K)


def _mp_frame(mp, S, d):
    """S * exp(d) to first order in v and sigma, exactly in w: R expm([w]x), t + s R v, s exp(sigma)."""
    R = _mp_rot(mp, S[:4])
    t, s = mp.matrix(S[4:7]), S[7]
    if any(d[3:6]):
        R = R * mp.expm(mp.matrix([[0, -d[5], d[4]], [d[5], 0, -d[3]], [-d[4], d[3], 0]]))
    if any(d[:3]):
        t = t + s * (_mp_rot(mp, S[:4]) * mp.matrix(d[:3]))
    return R, t, s * mp.exp(d[6])


def _mp_residual(mp, ob, delta):
    """The specification's residual at the state moved by delta = dj (7) + dh (7) + dlm (3) + dc (9); None: it does not exist."""
    f = lambda v: mp.mpf(float(v))
    Sj, Sh = [f(v) for v in ob["Sj"]], [f(v) for v in ob["Sh"]]
    Rj, tj, sj = _mp_frame(mp, Sj, delta[0:7])
    if ob["kind"] == 0:
        Z = mp.matrix([f(ob["lm"][e]) + delta[14 + e] for e in range(3)]) - tj
    else:
        Rh, th, sh = (Rj, tj, sj) if ob["same_host"] else _mp_frame(mp, Sh, delta[7:14])
        Z = sh * (Rh * mp.matrix([f(v) for v in ob["anchor"]])) + (f(ob["lm"][0]) + delta[14]) * (th - tj)
    Y = Rj.T * Z
    m = [f(v) for v in ob["m"]]
    if ob["projection"] == 0:
        if not Y[2] > f(gc.MIN_DEPTH):
            return None
        x, y = Y[0] / Y[2], Y[1] / Y[2]
        if ob["cam"] is None:
            return [x - m[0], y - m[1]]
        fx, fy, cx, cy, k1, k2, p1, p2, k3 = [f(ob["cam"][e]) + delta[17 + e] for e in range(9)]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        X1 = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        Y1 = y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
        return [cx + fx * X1 - m[0], cy + fy * Y1 - m[1]]
    n = mp.sqrt(Y[0] ** 2 + Y[1] ** 2 + Y[2] ** 2)
    if not n > f(gc.MIN_DEPTH):
        return None
    yv = [Y[e] / n for e in range(3)]
    if not yv[0] * m[0] + yv[1] * m[1] + yv[2] * m[2] > 0:
        return None
    k = [mp.mpf(1) if e == _axis(np.asarray(ob["m"], float)) else mp.mpf(0) for e in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    e1 = cross(m, k)
    n1 = mp.sqrt(e1[0] ** 2 + e1[1] ** 2 + e1[2] ** 2)
    e1 = [v / n1 for v in e1]
    e2 = cross(m, e1)
    return [sum(e1[e] * yv[e] for e in range(3)), sum(e2[e] * yv[e] for e in range(3))]


def _mp_lin(mp, ob):
    """-> None or (r 2, w, J 2 x 26: dj 7, dh 7, dlm 3, dc 9)"""
    zero = [mp.mpf(0)] * 26
    r = _mp_residual(mp, ob, zero)
    if r is None:
        return None
    h = mp.mpf(10) ** -20
    J = np.zeros((2, 26))
    cols = list(range(7)) + (list(range(7, 14)) if ob["kind"] == 1 and not ob["same_host"] else []) + (list(range(14, 17)) if ob["kind"] == 0 else [14])
    cols += list(range(17, 26)) if ob["cam"] is not None else []
    for c in cols if not ob["same_host"] else (list(range(17, 26)) if ob["cam"] is not None else []):
        up, dn = list(zero), list(zero)
        up[c], dn[c] = h, -h
        a, b = _mp_residual(mp, ob, up), _mp_residual(mp, ob, dn)
        J[:, c] = [float((a[e] - b[e]) / (2 * h)) for e in range(2)]
    f = lambda v: mp.mpf(float(v))
    L = [[1, 0], [0, 1]] if ob["info"] is None else [[f(ob["info"][0]), f(ob["info"][1])], [f(ob["info"][2]), f(ob["info"][3])]]
    s = r[0] * (L[0][0] * r[0] + L[0][1] * r[1]) + r[1] * (L[1][0] * r[0] + L[1][1] * r[1])
    d = f(ob["huber"])
    w = d / mp.sqrt(s) if d > 0 and s > d * d else mp.mpf(1)
    return np.array([float(r[0]), float(r[1])]), float(w), J


def observation(case, k, cls, **change):
    """Everything oracle_graph_obs takes for observation k of a case at its start."""
    pr = case["problem"]
    kind, point, frame, xy, info = pr["obs"]
    kd, p, j = int(kind[k]), int(point[k]), int(frame[k])
    h = int(pr["idp"][0][p]) if kd == 1 else j
    cam = pr.get("intrinsics")
    ob = {"cls": cls, "kind": kd, "Sj": case["start"][j], "Sh": case["start"][h], "same_host": kd == 1 and h == j,
          "lm": pr["xyz"][0][p] if kd == 0 else np.array([pr["idp"][2][p], 0.0, 0.0]), "anchor": pr["idp"][1][p] if kd == 1 else np.zeros(3), "m": xy[k],
          "info": None if info is None else info[k], "huber": case["huber"], "projection": 1 if pr.get("projection") == "sphere" else 0,
          "cam": None if cam is None else np.asarray(cam[0], np.float64)}
    ob.update(change)
    return ob


def _lin_inputs():
    C = gc.CASES
    out = [observation(C["base"], k, "base") for k in range(0, 160, 16)]
    out += [observation(C["depth_edge"], k, "depth_edge") for k in (160, 161, 162)]
    pr = C["rho_floor"]["problem"]
    low = [k for k in range(160) if pr["obs"][0][k] == 1 and pr["obs"][1][k] < 3 and pr["obs"][2][k] != pr["idp"][0][pr["obs"][1][k]]]
    out += [observation(C["rho_floor"], k, "rho_edges") for k in low[:5]] + [observation(C["rho_floor"], k, "rho_edges", lm=np.array([1e-9, 0, 0])) for k in low[5:8]]
    out += [observation(C["rho_huge"], k, "rho_edges") for k in low[:6]]
    pr = C["sim3_scales"]["problem"]
    scaled = [k for k in range(160) if pr["obs"][2][k] in gc.SCALES or (pr["obs"][0][k] == 1 and pr["idp"][0][pr["obs"][1][k]] in gc.SCALES)]
    out += [observation(C["sim3_scales"], k, "sim3_scales") for k in scaled[::6]]
    out += [observation(C["far_world"], k, "far_world") for k in range(3, 160, 20)]
    out += [observation(C["info_rank1_zero_scales"], k, "info") for k in np.flatnonzero(gc.INFO_SORT < 4)[::7]]
    out += [observation(C["huber_corner"], k, "huber_corner") for k in (160, 161, 162)]
    out += [observation(C["opposite_hemisphere"], k, "sphere") for k in list(range(0, 160, 24)) + list(range(5, 160, 40))]
    out += [observation(C["tangent_axis_ties"], k, "sphere") for k in range(160, 160 + len(gc.AXES))]
    far = np.flatnonzero(np.linalg.norm(_normalised(C["cam_fold_over"]), axis=1) > gc.FOLD_RADIUS)
    out += [observation(C["cam_fold_over"], k, "camera") for k in list(far[:5]) + [2, 82]]
    out += [observation(C["cam_unobservable"], k, "camera") for k in (0, 40, 80)]
    return out


def test_linearisation_against_mpmath(oracle):
    import mpmath as mp
    worst, missing, weights = {}, {}, []
    inputs = _lin_inputs()
    assert 80 <= len(inputs) <= 110
    with mp.workdps(50):
        for ob in inputs:
            a = (ob["kind"], ob["Sj"], 127, ob["Sh"], 127, ob["same_host"], ob["lm"], 1, ob["anchor"], ob["m"])
            if ob["cam"] is None:
                ok, r, w, s, Jj, Jh, Jp = oracle.graph_obs(*a, ob["info"], ob["huber"], ob["projection"])
                Jc = np.zeros((2, 9))
            else:
                ok, r, w, s, Jj, Jh, Jp, Jc = oracle.graph_obs_cam(*a, ob["cam"], 0x1FF, ob["info"], ob["huber"])
            ref = _mp_lin(mp, ob)
            assert bool(ok) == (ref is not None), (ob["cls"], ob["lm"], ob["m"])
            if ref is None:
                missing[ob["cls"]] = missing.get(ob["cls"], 0) + 1
                continue
            r_ref, w_ref, J = ref
            if ob["same_host"]:  # a constant: the residual of the anchor, no Jacobian towards the frame or the point
                assert not Jj.any() and not Jh.any() and not Jp.any()
            pairs = ((r, r_ref), (Jj, J[:, :7]), (Jh, J[:, 7:14]), (Jp, J[:, 14:17]), (Jc, J[:, 17:]), (np.array([w]), np.array([w_ref])))
            err = max([ULP] + [np.abs(x - y).max() / max(1.0, np.abs(y).max()) for x, y in pairs])
            worst[ob["cls"]] = max(worst.get(ob["cls"], 0.0), err)
            if ob["cls"] == "huber_corner":
                weights.append((s, w))
    print("worst linearisation error per class:", dict((k, "%.1e" % v) for k, v in sorted(worst.items())))
    print("observations that do not exist on both sides, per class:", missing)
    for cls, err in worst.items():
        assert err <= LIN_BAR[cls], (cls, err)
    assert sorted(worst) == sorted(LIN_BAR) and missing["depth_edge"] == 2 and missing["sphere"] >= 5 and missing.get("rho_edges", 0) >= 1
    h2 = gc.HUBER_CORNER * gc.HUBER_CORNER
    assert [s > h2 for s, _ in weights] == [False, False, True] and weights[1][0] == h2
    assert weights[0][1] == 1.0 and weights[1][1] == 1.0 and weights[2][1] < 1.0  # s == h^2 is still quadratic


# ------------------------------------------------------------------------------------------------ first LM step, dense
def _solve_spd_longdouble(A, b):
    """Gaussian elimination without pivoting (A is symmetric positive definite) in longdouble."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def dense_first_candidate(oracle, case, radius=1e4):
    """The first candidate of the LM loop without a Schur complement.  -> (start, dof, problem) of the candidate, H's diagonal"""
    pr = case["problem"]
    assert not any(k in pr for k in ("se3", "sim3", "gps"))
    S, dof = case["start"], case["dof"]
    xyz, xfree = pr["xyz"]
    host, anchor, rho, ifree = pr["idp"]
    cam = pr.get("intrinsics")
    col = {}
    for f in range(len(dof)):
        for k in range(7):
            if (int(dof[f]) >> k) & 1:
                col[("f", f, k)] = len(col)
    for p in range(len(xyz)):
        if xfree[p]:
            for k in range(3):
                col[("x", p, k)] = len(col)
    for p in range(len(rho)):
        if ifree[p]:
            col[("i", p, 0)] = len(col)
    for k in range(9):
        if cam is not None and (cam[1] >> k) & 1:
            col[("c", 0, k)] = len(col)
    n = len(col)
    H, g = np.zeros((n, n), np.longdouble), np.zeros(n, np.longdouble)
    for k in range(len(pr["obs"][0])):
        ob = observation(case, k, "")
        j, p = int(pr["obs"][2][k]), int(pr["obs"][1][k])
        h = int(host[p]) if ob["kind"] == 1 else j
        free = int(xfree[p]) if ob["kind"] == 0 else int(ifree[p])
        a = (ob["kind"], ob["Sj"], int(dof[j]), ob["Sh"], int(dof[h]), ob["same_host"], ob["lm"], free, ob["anchor"], ob["m"])
        if cam is None:
            ok, r, w, s, Jj, Jh, Jp = oracle.graph_obs(*a, ob["info"], ob["huber"], ob["projection"])
            Jc = np.zeros((2, 9))
        else:
            ok, r, w, s, Jj, Jh, Jp, Jc = oracle.graph_obs_cam(*a, cam[0], cam[1], ob["info"], ob["huber"])
        if not ok:
            continue
        keys = [("f", j, e) for e in range(7)] + [("f", h, e) for e in range(7)] + [("x" if ob["kind"] == 0 else "i", p, e) for e in range(3)] + [("c", 0, e) for e in range(9)]
        J = np.concatenate([Jj, Jh, Jp, Jc], axis=1)
        use = [e for e, key in enumerate(keys) if key in col and (e < 7 or e >= 14 or h != j)]
        assert not np.delete(J, use, axis=1).any(), "a Jacobian column towards an unknown that is fixed"
        idx = [col[keys[e]] for e in use]
        Ju = J[:, use].astype(np.longdouble)
        L = np.longdouble(w) * (np.eye(2) if ob["info"] is None else np.asarray(ob["info"]).reshape(2, 2)).astype(np.longdouble)
        H[np.ix_(idx, idx)] += Ju.T @ L @ Ju
        g[idx] += Ju.T @ (L @ r.astype(np.longdouble))
    diag = np.diag(H).copy()
    H[np.diag_indices(n)] += np.clip(diag, np.longdouble(1e-6), np.longdouble(1e32)) / np.longdouble(radius)
    step = _solve_spd_longdouble(H, -g).astype(np.float64)
    S1, xyz1, rho1 = S.copy(), np.array(xyz, dtype=np.float64), np.array(rho, dtype=np.float64)
    cam1 = None if cam is None else np.array(cam[0], dtype=np.float64)
    for f in range(len(dof)):
        if int(dof[f]) & 127:
            S1[f] = oracle.sim3_retract(S[f], np.array([step[col[("f", f, e)]] if ("f", f, e) in col else 0.0 for e in range(7)]))
    for (what, p, e), c in col.items():
        if what == "x":
            xyz1[p, e] += step[c]
        elif what == "i":
            rho1[p] = max(rho1[p] + step[c], gc.RHO_FLOOR)
        elif what == "c":
            cam1[e] += step[c]
    out = dict(pr, xyz=(xyz1, xfree), idp=(host, anchor, rho1, ifree))
    if cam is not None:
        out["intrinsics"] = (cam1, cam[1])
    return S1, dof, out, diag.astype(np.float64), col


@pytest.mark.parametrize("name", sorted(STEP_BAR))
def test_first_lm_step_without_schur(oracle, name):
    case = gc.CASES[name]
    radius = STEP_RADIUS.get(name, 1e4)
    S1, dof, pr1, diag, col = dense_first_candidate(oracle, case, radius)
    # what each case brings to the damping
    block = lambda what, p, k: np.array([diag[col[(what, p, e)]] for e in range(k)])
    if name == "lone_idp_host_only":
        assert all(diag[col[("i", p, 0)]] == 0 for p in range(gc.LONE)) and pr1["idp"][2][:gc.LONE].tobytes() == case["problem"]["idp"][2][:gc.LONE].tobytes()
    elif name == "unobserved_landmarks":
        assert (diag == 0).sum() == 3 * 3 + 3
    elif name == "first_nonhost_obs_invalid":
        assert not any(diag[col[("f", 6, e)]] for e in range(6))
    elif name == "cam_underdetermined":
        assert sum(1 for key in col if key[0] == "c") == 9 and len(case["problem"]["obs"][0]) == 3
    mine = oracle.graph_cost(S1, dof, pr1, case["huber"])
    got = solve(oracle, case, max_iterations=1, initial_radius=radius)
    sm = got["sm"]
    assert got["st"] == 0 and sm.trace_len == 1 and sm.trace_accepted[0] == 1 and sm.trace_radius[0] == radius
    rel = max(abs(mine - sm.trace_cost[0]) / sm.trace_cost[0], ULP)  # (a float64 cost cannot be compared finer than its last bit)
    print("%s: first candidate %.17g, dense longdouble step %.17g, relative difference %.1e" % (name, sm.trace_cost[0], mine, rel))
    assert rel <= STEP_BAR[name]


def test_the_rejected_step_puts_the_point_behind_its_camera(oracle):
    """step_pushes_behind: the dense first step moves the extra point to a depth of -0.01 in the identity keyframe (every other
    observation stays in front of its camera), and the oracle's first candidate costs inf."""
    case = gc.CASES["step_pushes_behind"]
    S1, dof, pr1, _, _ = dense_first_candidate(oracle, case)
    moved = dict(case, start=S1, problem=pr1)
    valid = gc.valid_at_start(moved)
    assert list(np.flatnonzero(~valid)) == [len(valid) - 1] and abs(pr1["xyz"][0][-1][2] + 0.01) < 1e-4
    sm = solve(oracle, case, max_iterations=1)["sm"]
    assert sm.trace_cost[0] == np.inf and sm.trace_accepted[0] == 0


# ------------------------------------------------------------------------------------------------ minimum
@pytest.mark.parametrize("name", sorted(MIN_BAR))
def test_the_minimum_is_scipys(oracle, name):
    from test_graph_oracle import _scipy_minimum
    case = gc.CASES[name]
    got = solve(oracle, case, max_iterations=80, function_tolerance=1e-14)
    ref_cost, _ = _scipy_minimum(oracle, case["start"], case["dof"], case["problem"])
    rel = abs(got["sm"].final_cost - ref_cost) / ref_cost
    print("%s: final cost %.17g, scipy %.17g, relative difference %.1e" % (name, got["sm"].final_cost, ref_cost, rel))
    assert got["st"] == 0 and rel <= MIN_BAR[name]


# ------------------------------------------------------------------------------------------------ yardstick
def measure_yardstick(oracle, fma, name):
    a, b = solve(oracle, gc.CASES[name]), solve(fma, gc.CASES[name])
    sa, sb = a["sm"], b["sm"]
    assert (a["st"], sa.iterations, sa.accepted, sa.termination, sa.trace_len) == (b["st"], sb.iterations, sb.accepted, sb.termination, sb.trace_len), name
    assert accepts(sa) == accepts(sb), name
    return state_difference(a, b), cost_difference(sa, sb)


def test_yardstick(oracle):
    fma = oracle_lib.Oracle(os.path.join(oracle_lib.ROOT, "oracle", "liboracle_fma.so"))
    assert sorted(gc.YARDSTICK) == sorted(gc.FINITE)
    within = lambda got, rec: (got == 0.0 and rec == 0.0) or 0.5 * rec <= got <= 2.0 * rec
    for name in gc.FINITE:
        got, rec = measure_yardstick(oracle, fma, name), gc.YARDSTICK[name]
        print('    "%s": (%.2e, %.2e),' % (name, got[0], got[1]))
        assert within(got[0], rec[0]) and within(got[1], rec[1]), (name, got, rec)
