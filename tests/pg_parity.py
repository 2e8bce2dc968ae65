"""The parity bars of the pose-graph solver against oracle/pg_oracle.c, shared by tests/test_pg_gpu.py and
tests/test_pg_adversarial_gpu.py: initial cost 1e-12 relative; identical LM iteration count, termination and accept /
reject sequence; per-iteration radius and cost 1e-9 relative; keyframes 1e-7; the fixed frames bit-identical (reasoning
in the docstring of tests/test_pg_gpu.py)."""
import numpy as np

import oracle_lib


def compare_runs(got, ref, start, fixed=(0,)):
    """(frames, summary, status) of a run against a reference run of the same problem."""
    Sg, sg, stg = got
    So, so, sto = ref
    assert stg == sto == 0
    assert abs(sg.initial_cost - so.initial_cost) <= 1e-12 * max(so.initial_cost, 1e-30)
    assert (sg.iterations, sg.accepted, sg.termination, sg.trace_len) == (so.iterations, so.accepted, so.termination, so.trace_len)
    for i in range(so.trace_len):
        assert sg.trace_accepted[i] == so.trace_accepted[i], i
        assert abs(sg.trace_radius[i] - so.trace_radius[i]) <= 1e-9 * so.trace_radius[i]
        assert abs(sg.trace_cost[i] - so.trace_cost[i]) <= 1e-9 * max(so.trace_cost[i], 1e-30) + 1e-20
    assert np.abs(Sg - So).max() <= 1e-7
    for f in fixed:
        assert Sg[f].tobytes() == start[f].tobytes()


def compare(ctx, oracle, truth, start, dof, prob, max_it=40, fixed=(0,), solve=None):
    """The GPU solve of a problem against the oracle's.  fixed = the frames that must come back bit-identical (frame 0 in
    the graphs of make_pose_graph); solve(ctx, start, dof, prob, options) -> (frames, summary, status), by default
    gslam_amd.posegraph.solve."""
    from gslam_amd import ba, posegraph
    ref = oracle.pg_solve(start, dof, prob, oracle_lib.ba_options(max_iterations=max_it), threads=4)
    got = (solve or posegraph.solve)(ctx, start, dof, prob, ba.default_options(max_iterations=max_it))
    compare_runs(got, ref, start, fixed)
    return got[0], got[1]
