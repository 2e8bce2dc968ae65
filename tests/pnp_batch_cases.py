"""Inputs of the batched pose refinement tests (tests/test_pnp_batch_gpu.py).  Every problem comes from the generator the
PnP tests of tests/test_full_configs_gpu.py use (make_graph(3, n, ...), camera 1, start = the truth retracted by START_XI);
the problems are concatenated into one segmented batch.  Sizes sit on and around the kernel's 256-thread stride (1, 3, 6,
255, 256, 257, 513 participating rows), masks on its 64-row wave and 256-row chunk boundaries."""
import functools

import numpy as np

from gslam_amd.ba_synth import make_graph

START_XI = np.array([0.05, -0.04, 0.03, 0.01, -0.02, 0.015])
FILL_DOUBLE, FILL_BYTE, FILL_INT = 7.0, 0xAB, -5
PAD_ROWS = 5           # rows behind offsets[nproblems]: they belong to nobody
INLIER_THRESHOLD = 0.006


def pnp_case(oracle, seed, n_pts, noise, outlier_every):
    """-> X n x 3, m n x 2, start 7, displacement n x 2 (zeros where the observation was not displaced)."""
    g = make_graph(3, n_pts, n_obs_per_point=3, seed=seed, noise=0.0, outlier_frac=0.0, perturb=False)
    sel = g["obs_cam"] == 1
    X = g["point_xyz_gt"][g["obs_point"][sel]]
    rng = np.random.default_rng(seed)
    m = g["obs_xy"][sel] + rng.standard_normal((int(sel.sum()), 2)) * noise
    disp = np.zeros_like(m)
    if outlier_every:
        disp[::outlier_every] = rng.standard_normal((len(m[::outlier_every]), 2)) * 0.1
        m = m + disp
    start = oracle.se3_retract(g["cam_pose_gt"][1], START_XI)
    return np.ascontiguousarray(X), np.ascontiguousarray(m), start, disp


def _mask(kind, n):
    m = np.zeros(n, np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "odd":
        m[1::2] = 1
    elif kind == "last":
        m[-1] = 1
    elif kind == "straddle":       # set rows on both sides of a wave boundary (64) and of a chunk boundary (256)
        m[60:71] = 1
        m[250:263] = 1
    elif kind == "edges":          # the last lane of a wave / chunk and the first of the next, nothing else
        m[[63, 64, 255, 256, 511, 512]] = 1
    elif kind == "hole":           # everything but waves 1 .. 3 of the first chunk
        m[:] = 1
        m[64:256] = 0
    elif kind == "random":
        m[:] = np.random.default_rng(n).random(n) < 0.7
    elif kind == "values":         # any non-zero byte counts
        m[:] = np.arange(n) % 3
    else:
        raise ValueError(kind)
    return m


# (rows of the range, mask kind) -> participating rows under the mask
CENSUS = [(1, "ones"), (3, "ones"), (6, "ones"), (255, "ones"), (256, "ones"), (257, "ones"), (513, "ones"),
          (12, "alternating"), (510, "alternating"), (512, "alternating"), (514, "odd"), (1026, "alternating"),
          (300, "last"), (257, "last"), (600, "straddle"), (700, "edges"), (520, "hole"), (400, "random"), (90, "values"),
          (2, "last"), (64, "ones"), (769, "alternating"), (512, "ones")]


@functools.lru_cache(maxsize=None)
def _census(oracle):
    X, m, mask, starts, names = [], [], [], [], []
    offsets = [0]
    for p, (n, kind) in enumerate(CENSUS):
        Xp, mp, start, _ = pnp_case(oracle, 100 + p, n, 0.002, 7)
        assert len(Xp) == n
        X.append(Xp)
        m.append(mp)
        mask.append(_mask(kind, n))
        starts.append(start)
        names.append("%s_%d" % (kind, n))
        offsets.append(offsets[-1] + n)
    X.append(X[0][:1].repeat(PAD_ROWS, 0))
    m.append(m[0][:1].repeat(PAD_ROWS, 0))
    mask.append(np.ones(PAD_ROWS, np.uint8))
    return dict(X=np.concatenate(X), m=np.concatenate(m), mask=np.concatenate(mask), starts=np.array(starts),
                offsets=np.array(offsets, np.int32), names=names)


def census(oracle):
    """The batch of test (1): dict of host arrays X, m, mask (rows + PAD_ROWS), starts P x 7, offsets P + 1, names."""
    return _census(oracle)


# what one call fixes for all its problems: Huber delta, dof, iteration limit, information asked for, mask given
CONFIGS = {"huber_se3_info_mask": dict(huber=0.01, dof=63, max_iterations=50, info=True, mask=True),
           "plain_se3_mask": dict(huber=0.0, dof=63, max_iterations=50, info=False, mask=True),
           "huber_rotation_info_nomask": dict(huber=0.01, dof=0b111000, max_iterations=50, info=True, mask=False),
           "huber_translation_mask": dict(huber=0.01, dof=0b000111, max_iterations=50, info=False, mask=True),
           "no_iterations_info_mask": dict(huber=0.01, dof=63, max_iterations=0, info=True, mask=True),
           "huber_se3_nomask": dict(huber=0.01, dof=63, max_iterations=50, info=False, mask=False)}


def rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def model_of_pose(pose):
    """T_wc pose -> the estimator's [R row-major | t] with X_cam = R X + t."""
    R = rotation(pose[:4]).T
    return np.concatenate([R.ravel(), -R @ pose[4:]])
