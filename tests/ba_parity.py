"""GPU bundle adjustment against the oracle at the full-size bars: identical accept / reject sequence, cost 1e-9,
state 1e-8, and the oracle's cost AT the GPU's state equal to the GPU's reported final cost.  A plain helper module (not a
conftest.py): tests/test_full_configs_gpu.py and tests/test_ba_solver_paths_gpu.py import it.

Full-size bars = the bars of the small graphs.  Rounds 1-3 had to loosen the state to 1e-5 because their generator left 300 of
500 cameras unobserved; on the co-visibility-window graphs of gslam_amd/ba_synth.py the oracle compiled with and
without FMA contraction differs from itself by 1e-11 in pose (tests/test_ba_oracle.py::test_full_c4_state_sensitivity_to_rounding,
CPU), and the oracle on a camera-shuffled graph by 1e-12 .. 1e-10 (test_ba_oracle.py::test_full_c4_oracle_camera_order_sensitivity)."""
import os

import numpy as np

import oracle_lib

STATE_ATOL_FULL = 1e-8
RADIUS_RTOL_FULL = 1e-9
COST_RTOL = 1e-9
STATE_ATOL = 1e-8
THREADS = max(1, min(32, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def _compare_ba(oracle, ctx, g, max_it, huber=0.01, state_atol=STATE_ATOL_FULL, radius_rtol=RADIUS_RTOL_FULL, eo=None):
    """eo: the oracle's (poses, points, summary, status) for (g, huber, max_it) when the caller already has it"""
    from gslam_amd import ba
    if eo is None:
        eo = oracle.ba_solve(g, oracle_lib.ba_options(huber=huber, max_iterations=max_it), threads=THREADS)
    gp = ba.solve(ctx, g, ba.default_options(huber_delta=huber, max_iterations=max_it, deterministic=1))
    so, sg = eo[2], gp[2]
    assert gp[3] == 0 and eo[3] == 0
    assert abs(sg.initial_cost - so.initial_cost) <= COST_RTOL * so.initial_cost
    assert (sg.iterations, sg.accepted, sg.termination, sg.trace_len) == (so.iterations, so.accepted, so.termination,
                                                                         so.trace_len)
    for i in range(so.trace_len):
        assert sg.trace_accepted[i] == so.trace_accepted[i], f"accept/reject differs at iteration {i}"
        assert abs(sg.trace_radius[i] - so.trace_radius[i]) <= radius_rtol * so.trace_radius[i]
        if np.isinf(so.trace_cost[i]):  # candidate rejected: it moved an observation behind its camera
            assert np.isinf(sg.trace_cost[i])
            continue
        assert abs(sg.trace_cost[i] - so.trace_cost[i]) <= COST_RTOL * so.trace_cost[i], f"cost at iteration {i}"
    assert abs(sg.final_cost - so.final_cost) <= COST_RTOL * so.final_cost
    assert np.abs(gp[0] - eo[0]).max() <= state_atol
    assert np.abs(gp[1] - eo[1]).max() <= state_atol
    # the returned state is self-consistent: the oracle's cost AT the GPU's state is the GPU's reported final cost
    assert abs(oracle.ba_cost(g, gp[0], gp[1], huber=huber) - sg.final_cost) <= 1e-12 * sg.final_cost
    return so
