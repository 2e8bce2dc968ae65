"""The two-view entries (gh_two_view_batch_dev, gh_two_view_pairs_dev, gh_two_view_default_params) are declared, exported and
mirrored; the scalar restatement of their contract (tests/two_view_restate.py) recovers ground truth, so a convention
error shared by kernel and restatement cannot hide; and the inputs tests/test_two_view_gpu.py runs on the device reach every
candidate, every status and every per-row test (their census, taken with the restatement).  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import two_view_cases as tc
import two_view_restate as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gh_two_view_batch_dev", "gh_two_view_pairs_dev", "gh_two_view_default_params")


def test_entries_are_declared_and_exported():
    from gslam_amd import estimator, hip
    raw = open(os.path.join(ROOT, "include", "gslam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in hip.SIGNATURES and name not in hip.bind(strict=False)
        assert getattr(hip.lib, name) is not None
    for k, name in enumerate(("OK", "NO_MODEL", "TOO_FEW", "AMBIGUOUS")):
        assert re.search(r"#define\s+GH_TWO_VIEW_%s\s+%d\b" % (name, k), src), name
        assert getattr(estimator, "TWO_VIEW_" + name) == k == getattr(tv, name)
    assert "gh_two_view_params" in src
    for name in ("two_view_batch", "two_view_pairs", "two_view_default_params"):
        assert callable(getattr(estimator, name)), name
    assert hip.lib.gh_abi_version() == 2  # entries were added, none changed meaning


def test_default_params_and_layout():
    from gslam_amd import estimator, hip
    assert C.sizeof(hip.TwoViewParams) == 24
    p = estimator.two_view_default_params()
    got = dict(min_parallax_cos=p.min_parallax_cos, max_reproj=p.max_reproj, min_good=p.min_good,
               min_good_permille=p.min_good_permille)
    assert got == tv.DEFAULTS == dict(min_parallax_cos=0.99998, max_reproj=0.004, min_good=50, min_good_permille=900)


def _pose_error(pose, R, t):
    Rg = np.array(tv.rotation_of(pose[:4])).reshape(3, 3)
    return max(np.abs(Rg - R).max(), np.abs(np.array(pose[4:]) - t / np.linalg.norm(t)).max())


def test_restatement_recovers_ground_truth():
    """Noise-free views of tests/test_ransac_oracle.py's _two_view geometry: R, t / |t| to 1e-8 and the points to 1e-7
    relative of X / |t| (the BA tolerances of SURVEY section 8c; a sign or transpose error is O(1)).  Measured: 1e-16 and
    9e-14.  Both signs of E and of t, so every candidate index is the right answer once."""
    winners = set()
    for t in (tc.T_TRUE, -tc.T_TRUE):
        src, dst, X = tc.scene(200, 1, t=t)
        for sign in (1.0, -1.0):
            r = tv.two_view((sign * tc.essential(tc.R_TRUE, t)).tolist(), src, dst)
            assert r["status"] == tv.OK and r["counts"][r["best"]] == 200 == r["n_used"] == sum(r["good"])
            assert sum(r["counts"]) == 200  # no row is good under a wrong candidate
            q = r["pose"][:4]
            assert abs(sum(e * e for e in q) - 1.0) < 1e-15 and q[3] >= 0
            assert abs(sum(e * e for e in r["pose"][4:]) - 1.0) < 1e-15
            assert _pose_error(r["pose"], tc.R_TRUE, t) <= 1e-8
            want = X / np.linalg.norm(t)
            rel = np.linalg.norm(np.array(r["points"]) - want, axis=1) / np.linalg.norm(want, axis=1)
            assert rel.max() <= 1e-7, rel.max()
            winners.add(r["best"])
    assert winners == {0, 1, 2, 3}


def test_quaternion_pivots():
    """Shepperd's four branches: rotations by ~pi about x, y, z take the diagonal pivots; all give back their matrix."""
    picks = set()
    for axis, ang in (([1, 0, 0], 3.0), ([0, 1, 0], 3.1), ([0, 0, 1], 2.9), ([1, 2, 3], 0.4), ([1, 1, 0], 3.14)):
        R = tc.rot(axis, ang).reshape(9).tolist()
        q = tv.quat(R)
        assert q[3] >= 0 and np.abs(np.array(tv.rotation_of(q)) - np.array(R)).max() < 1e-14
        tr = R[0] + R[4] + R[8]
        picks.add(int(np.argmax([tr, R[0], R[4], R[8]])))
    assert picks == {0, 1, 2, 3}


def test_census_of_the_gpu_batch():
    a, ex = tc.batch_arrays(9), tc.batch_expected()
    by = dict(zip(a["names"], ex["results"]))
    sizes = {n: by["rows_%d" % n] for n in tc.ROW_COUNTS}
    assert all(r["n_used"] == n for n, r in sizes.items())
    assert {r["best"] for n, r in sizes.items() if r["status"] == tv.OK} == {0, 1, 2, 3}
    assert set(ex["status"]) == {tv.OK, tv.NO_MODEL, tv.TOO_FEW, tv.AMBIGUOUS}
    for name in ("zero_E", "nan_E", "rank1_E"):
        assert by[name]["status"] == tv.NO_MODEL and by[name]["n_used"] == 20 and by[name]["counts"] == [0, 0, 0, 0], name
    for name in ("empty_first", "empty_middle", "empty_last", "mask_zero", "reversed", "overlap_zero_E", "past_the_end",
                 "from_past_the_end", "negative_begin"):
        assert by[name]["status"] == tv.NO_MODEL and by[name]["n_used"] == 0, name
    assert a["names"][0] == "empty_first" and a["names"].index("empty_middle") not in (0, len(a["names"]) - 1)
    assert by["far_scene"]["status"] == tv.TOO_FEW and by["far_scene"]["counts"] == [0, 0, 0, 0]
    assert all(tv.PARALLAX in r for r in by["far_scene"]["reasons"])  # under the true candidate parallax fails every row
    assert by["rows_1"]["status"] == tv.TOO_FEW and max(by["rows_1"]["counts"]) == 1      # by min_good
    low = by["low_share"]
    assert low["status"] == tv.TOO_FEW and max(low["counts"]) >= tc.BATCH_PARAMS["min_good"]  # by the share alone
    # both sides of the 7 / 10 rule, and a tie
    assert by["mix_10_7"]["status"] == tv.OK and sorted(by["mix_10_7"]["counts"]) == [0, 0, 7, 10]
    assert by["mix_10_8"]["status"] == tv.AMBIGUOUS and sorted(by["mix_10_8"]["counts"]) == [0, 0, 8, 10]
    tie = by["mix_50_50"]
    assert tie["status"] == tv.AMBIGUOUS and sorted(tie["counts"]) == [0, 0, 50, 50] and tie["best"] == tie["counts"].index(50)
    holes = by["mask_holes"]
    assert holes["status"] == tv.OK and 0 < holes["n_used"] < 257 and sum(holes["good"]) == holes["n_used"]
    dirty = by["dirty_rows"]
    assert dirty["status"] == tv.OK and 200 < sum(dirty["good"]) < 300
    assert by["not_essential"]["status"] == tv.OK and by["before_reversed"]["status"] == tv.OK
    # every per-row test of the contract rejects some row somewhere
    seen = {code for r in ex["results"] for row in r["reasons"] if row for code in row}
    assert seen == {tv.GOOD, tv.PARALLEL, tv.BEHIND_RAY, tv.PARALLAX, tv.DEPTH, tv.REPROJ}
    # rows nobody owns keep the fill; rows of problems that are not OK are zero
    assert ex["good"][-1] == tc.FILL_GOOD and ex["points"][-1] == [tc.FILL_POINT] * 3
    off = a["offsets"]
    k = a["names"].index("mix_50_50")
    assert not any(ex["good"][off[k]:off[k + 1]]) and all(p == [0.0, 0.0, 0.0] for p in ex["points"][off[k]:off[k + 1]])
    # no output of the batch holds a NaN: the byte comparison on the device has no payload to argue about
    assert not np.isnan(np.array(ex["points"])).any() and not np.isnan(np.array(ex["poses"])).any()


def test_pair_rows_by_hand():
    """correspondences_from_matches plus the normalisation in numpy float64 gives the rows the pair entry fits."""
    from gslam_amd import estimator
    from gslam_amd.orb import KP_DTYPE
    cap = 5
    kps = np.zeros((2, cap), KP_DTYPE)
    kps["x"][0] = [320, 330, 345, 0, 14]
    kps["y"][0] = [240, 189, 291, 0, 24]
    kps["x"][1] = [820, 321, 32, 33, 34]
    kps["y"][1] = [240, 750, 42, 43, 44]
    counts = np.array([3, 2], np.int32)
    idx1 = np.array([[1, 0, 2, 0, 0],      # pair (0, 1): rows 0 -> 1 and 1 -> 0; row 2 dropped (2 >= counts[1]); rows 3, 4 past counts[0]
                     [2, -1, 0, 0, 0]], np.int32)  # pair (1, 0): row 0 -> 2; row 1 dropped (-1)
    corr = estimator.correspondences_from_matches(kps, counts, np.array([0, 1], np.int32), np.array([1, 0], np.int32), idx1, None)
    (s0, d0, r0), (s1, d1, r1) = corr
    assert r0.tolist() == [0, 1] and r1.tolist() == [0]
    # fx = 500, fy = 510, cx = 320, cy = 240
    assert tc.normalise(s0).tolist() == [[0.0, 0.0], [10 / 500, -51 / 510]]
    assert tc.normalise(d0).tolist() == [[1 / 500, 510 / 510], [500 / 500, 0.0]]
    assert tc.normalise(s1).tolist() == [[1.0, 0.0]] and tc.normalise(d1).tolist() == [[25 / 500, 51 / 510]]
    assert tc.normalise(s0).dtype == np.float64


def test_pair_composition_meets_the_pose_bound(oracle):
    """What tests/test_two_view_gpu.py will ask of the device, checked here first with the CPU oracle's essential fit and the
    restatement: at the noise of the pair test (the float32 rounding of the keypoint records, about 6e-8 normalised; nothing
    is added) the true pair and its reverse come back OK with the generator's pose to 1e-6."""
    from gslam_amd import estimator
    kps, counts, idx1, keep = tc.pair_frames()
    pq, pt = (np.array([p[k] for p in tc.PAIRS], np.int32) for k in (0, 1))
    corr = estimator.correspondences_from_matches(kps, counts, pq, pt, idx1, keep)
    assert [len(r) for _, _, r in corr][2:] == [0, 0] and min(len(corr[0][2]), len(corr[1][2])) > 200
    truth = ((tc.R_PAIR, tc.T_PAIR), (tc.R_PAIR.T, -tc.R_PAIR.T @ tc.T_PAIR))
    for p in (0, 1):
        src, dst = tc.normalise(corr[p][0]), tc.normalise(corr[p][1])
        m, mask, cnt, _ = oracle.estimate_ex(4, src, dst, tc.PAIR_THR, 0, confidence=1.0, seed=tc.PAIR_SEED)
        assert 150 < cnt < len(src)  # the wrong matches are out
        r = tv.two_view(m[:9].tolist(), src.tolist(), dst.tolist(), mask.tolist())
        assert r["status"] == tv.OK and r["n_used"] == cnt and sum(r["good"]) >= 0.9 * cnt
        err = _pose_error(r["pose"], *truth[p])
        print("pair", tc.PAIRS[p], "inliers", cnt, "pose error %.3e" % err)
        assert err <= 1e-6, err
