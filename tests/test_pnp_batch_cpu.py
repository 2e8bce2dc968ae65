"""gh_pnp_pose_from_model (host only: no GPU needed) against the scalar restatement tests/pnp_restate.py, byte for byte, and
against ground truth; the layout of gh_pnp_batch_summary."""
import ctypes as C

import numpy as np

import pnp_restate as pr
import two_view_restate as tv


def _convert(model):
    from gslam_amd import hip
    m = np.ascontiguousarray(model, dtype=np.float64)
    pose = np.full(7, 7.0)
    ok = hip.lib.gh_pnp_pose_from_model(m.ctypes.data_as(C.c_void_p), pose.ctypes.data_as(C.c_void_p))
    return pose, ok


def _random_models(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        R = np.array(tv.rotation_of(q.tolist())).reshape(3, 3)
        out.append(np.concatenate([R.ravel(), rng.standard_normal(3) * 5.0]))
    return out


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def test_conversion_equals_the_restatement_byte_for_byte():
    models = _random_models(200, 7)
    # the four Shepperd branches: the trace (identity) and each diagonal entry (rotations by pi about x, y, z) as the pivot
    models += [np.concatenate([R.ravel(), [0.3, -1.5, 2.0]]) for R in (np.eye(3), _rot(0, np.pi), _rot(1, np.pi), _rot(2, np.pi))]
    picks = set()
    for m in models:
        got, ok = _convert(m)
        want, want_ok = pr.pose_from_model(m.tolist())
        assert ok == 1 and want_ok
        assert got.tobytes() == np.array(want).tobytes(), (m, got, want)
        Rt = m[:9].reshape(3, 3).T.ravel()
        picks.add(int(np.argmax([Rt[0] + Rt[4] + Rt[8], Rt[0], Rt[4], Rt[8]])))
    assert picks == {0, 1, 2, 3}


def test_no_start_returns_zero_and_zeros():
    base = _random_models(1, 3)[0]
    nan, inf, inf_t = base.copy(), base.copy(), base.copy()
    nan[4], inf[2], inf_t[10] = np.nan, np.inf, -np.inf
    for m in (np.zeros(12), nan, inf, inf_t):
        got, ok = _convert(m)
        want, want_ok = pr.pose_from_model(m.tolist())
        assert ok == 0 and not want_ok
        assert got.tobytes() == np.zeros(7).tobytes() == np.array(want).tobytes(), (m, got)


def test_conversion_against_ground_truth():
    """R(q)^T == R and R t_wc + t == 0 to 1e-12."""
    for m in _random_models(200, 11):
        pose, ok = _convert(m)
        assert ok == 1
        R, t = m[:9].reshape(3, 3), m[9:]
        Rq = np.array(tv.rotation_of(pose[:4].tolist())).reshape(3, 3)
        assert abs(np.linalg.norm(pose[:4]) - 1.0) <= 1e-15 and pose[3] >= 0.0
        assert np.abs(Rq.T - R).max() <= 1e-12
        assert np.abs(R @ pose[4:] + t).max() <= 1e-12


def test_summary_layout_and_signatures():
    from gslam_amd import estimator, hip
    assert C.sizeof(hip.PnpBatchSummary) == 32 == estimator.SUMMARY_DTYPE.itemsize
    assert hip.PnpBatchSummary.initial_cost.offset == 16 and hip.PnpBatchSummary.final_cost.offset == 24
    assert (estimator.PNP_NO_START, estimator.PNP_TOO_FEW) == (4, 5)
    for name in ("gh_pnp_pose_from_model", "gh_pnp_refine_batch_dev", "gh_pnp_batch_dev"):
        assert name in hip.SIGNATURES and name not in hip.MISSING
    pose, ok = estimator.pnp_pose_from_model(np.concatenate([np.eye(3).ravel(), [1.0, 2.0, 3.0]]))
    assert ok and pose.tolist() == [0.0, 0.0, 0.0, 1.0, -1.0, -2.0, -3.0]
