"""The batched estimator entries (gh_ransac_batch_dev, gh_ransac_pairs_dev, gh_ransac_batch_tile_rows) are declared,
exported and mirrored, and the numpy restatement of the pair entry's gather rule does what the header says.  No GPU."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gh_ransac_batch_dev", "gh_ransac_pairs_dev", "gh_ransac_batch_tile_rows")


def test_entries_are_declared_and_exported():
    from gslam_amd import hip
    src = open(os.path.join(ROOT, "include", "gslam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in hip.SIGNATURES and name not in hip.bind(strict=False)
        assert getattr(hip.lib, name) is not None
    assert hip.lib.gh_abi_version() == 2  # entries were added, none changed meaning


def test_mirror_exposes_the_batch_functions():
    from gslam_amd import estimator
    for name in ("estimate_batch", "estimate_pairs", "correspondences_from_matches", "batch_tile_rows"):
        assert callable(getattr(estimator, name)), name


def test_tile_rows():
    from gslam_amd import estimator, hip
    for model in range(8):
        assert hip.lib.gh_ransac_batch_tile_rows(model) > 0
        assert estimator.batch_tile_rows(model) == hip.lib.gh_ransac_batch_tile_rows(model)
        # a tile of the widest rows stays inside the 64 KB a workgroup gets without asking for more
        assert estimator.batch_tile_rows(model) * 6 * 8 <= 65536
    for model in (-1, 8):
        assert hip.lib.gh_ransac_batch_tile_rows(model) <= 0


def test_correspondences_from_matches_by_hand():
    from gslam_amd import estimator
    from gslam_amd.orb import KP_DTYPE
    cap = 5
    kps = np.zeros((2, cap), KP_DTYPE)
    kps["x"][0] = [10, 11, 12, 13, 14]
    kps["y"][0] = [20, 21, 22, 23, 24]
    kps["x"][1] = [30, 31, 32, 33, 34]
    kps["y"][1] = [40, 41, 42, 43, 44]
    counts = np.array([4, 3], np.int32)        # query row 4 and train rows 3, 4 are not valid
    pair_q, pair_t = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    #                 pair 0: row 0 -> 2, row 1 dropped (-1), row 2 dropped (3 >= counts[1]), row 3 -> 0 but keep has a hole,
    #                         row 4 is past counts[0] whatever it says
    idx1 = np.array([[2, -1, 3, 0, 1],
                     [3, 0, 4, 9, 9]], np.int32)  # pair 1: row 0 -> 3, row 1 -> 0, row 2 dropped (4 >= counts[0])
    keep = np.array([[1, 1, 1, 0, 1],
                     [1, 1, 1, 1, 1]], np.uint8)
    (s0, d0, r0), (s1, d1, r1) = estimator.correspondences_from_matches(kps, counts, pair_q, pair_t, idx1, keep)
    assert r0.tolist() == [0] and s0.tolist() == [[10.0, 20.0]] and d0.tolist() == [[32.0, 42.0]]
    assert r1.tolist() == [0, 1] and s1.tolist() == [[30.0, 40.0], [31.0, 41.0]] and d1.tolist() == [[13.0, 23.0], [10.0, 20.0]]
    assert s0.dtype == d0.dtype == np.float64
    # without the mask the hole comes back, in ascending row order
    (s0, d0, r0), _ = estimator.correspondences_from_matches(kps, counts, pair_q, pair_t, idx1, None)
    assert r0.tolist() == [0, 3] and d0.tolist() == [[32.0, 42.0], [30.0, 40.0]]
    # the float32 view of the records (what the extractor hands out) gives the same rows
    view = kps.view(np.float32).reshape(2, cap, 7)
    (s0v, d0v, r0v), _ = estimator.correspondences_from_matches(view, counts, pair_q, pair_t, idx1, None)
    assert r0v.tolist() == [0, 3] and s0v.tobytes() == s0.tobytes() and d0v.tobytes() == d0.tobytes()
    # an empty query frame gives an empty problem with the right shape
    (se, de, re_), = estimator.correspondences_from_matches(kps, np.array([0, 3], np.int32), pair_q[:1], pair_t[:1], idx1[:1], None)
    assert se.shape == de.shape == (0, 2) and re_.shape == (0,)
