"""The parts of the batched pose refinement (gh_pnp_refine_batch_dev, include/gslam_hip.h) that have a closed form, restated
in scalar IEEE doubles: Python floats, + - * / and math.sqrt only, every sum in a stated order, as tests/two_view_restate.py
does for the two-view contract.  It shares no code with the library; the device is held to it bit for bit.
  pose_from_model  gh_pnp_pose_from_model: [R row-major | t] -> T_wc [qx qy qz qw tx ty tz], or no start;
  start_ok         the rule for a 7-double start;
  classify_row     the inlier rule of the last pass (the conjugate-quaternion rotation of the linearisation)."""
import two_view_restate as tv

MIN_DEPTH = 1e-9  # kMinDepth of the linearisation


def _finite(x):
    return x - x == 0.0


def start_ok(pose):
    """Every value finite and the quaternion's sum of squares > 0."""
    if not all(_finite(v) for v in pose):
        return False
    return pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3] > 0.0


def pose_from_model(m):
    """-> (pose7, ok).  q = quat(R^T) by Shepperd's rule, t_wc[i] = -((R[i] t0 + R[3 + i] t1) + R[6 + i] t2).  No start (zeros):
    a value that is not finite, R all zero (the estimator's "no model"), or a converted pose that fails start_ok."""
    m = [float(v) for v in m]
    finite = all(_finite(v) for v in m)
    zero = all(v == 0.0 for v in m[:9])
    Rt = [m[0], m[3], m[6], m[1], m[4], m[7], m[2], m[5], m[8]]
    t = m[9:12]
    pose = tv.quat(Rt) + [-((m[i] * t[0] + m[3 + i] * t[1]) + m[6 + i] * t[2]) for i in range(3)]
    if finite and not zero and start_ok(pose):
        return pose, True
    return [0.0] * 7, False


def quat_rotate(q, p):
    uvx = q[1] * p[2] - q[2] * p[1]
    uvy = q[2] * p[0] - q[0] * p[2]
    uvz = q[0] * p[1] - q[1] * p[0]
    uvx += uvx
    uvy += uvy
    uvz += uvz
    return [p[0] + q[3] * uvx + (q[1] * uvz - q[2] * uvy),
            p[1] + q[3] * uvy + (q[2] * uvx - q[0] * uvz),
            p[2] + q[3] * uvz + (q[0] * uvy - q[1] * uvx)]


def classify_row(pose, X, m, threshold):
    """1 when the point is in front of the camera (depth > 1e-9) and dx * dx + dy * dy <= threshold^2, else 0."""
    qc = [-pose[0], -pose[1], -pose[2], pose[3]]
    d = [X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]]
    Xc = quat_rotate(qc, d)
    if not (Xc[2] > MIN_DEPTH):
        return 0
    iz = 1.0 / Xc[2]
    dx = Xc[0] * iz - m[0]
    dy = Xc[1] * iz - m[1]
    return 1 if dx * dx + dy * dy <= threshold * threshold else 0


def classify(pose, X, m, threshold):
    """The rows of one problem -> list of 0 / 1.  pose: 7 floats; X: n x 3, m: n x 2 (nested lists of floats)."""
    pose = [float(v) for v in pose]
    return [classify_row(pose, [float(v) for v in x], [float(v) for v in y], float(threshold)) for x, y in zip(X, m)]
