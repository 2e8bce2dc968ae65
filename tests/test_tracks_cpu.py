"""gh_triangulate_tracks_dev without a GPU: the entries are declared, exported and mirrored; the census inputs of
tests/tracks_cases.py reach what they were built for (taken with the scalar restatement tests/tracks_restate.py, which
tests/test_tracks_gpu.py holds the device to bit for bit); the restatement recovers ground truth and agrees with an
independent two-ray formula."""
import ctypes as C
import os
import re

import numpy as np

import tracks_cases as tc
import tracks_restate as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_mirrored():
    from gslam_amd import estimator, hip
    header = open(os.path.join(ROOT, "include", "gslam_hip.h")).read()
    for name in ("gh_track_default_params", "gh_track_group_lanes", "gh_triangulate_tracks_dev"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.SIGNATURES and name not in hip.MISSING
        assert getattr(hip.lib, name) is not None
    assert header.index("gh_pnp_batch_dev(") < header.index("gh_triangulate_tracks_dev(")  # after the PnP batch entries
    assert C.sizeof(hip.TrackParams) == 24
    p = estimator.track_default_params()
    assert (p.min_parallax_cos, p.max_reproj, p.min_views, p.max_drops) == (0.9998, 0.004, 2, 2)
    assert tr.DEFAULTS == dict(min_parallax_cos=0.9998, max_reproj=0.004, min_views=2, max_drops=2)
    assert hip.lib.gh_track_group_lanes() == 8 == estimator.track_group_lanes() == tr.LANES
    assert hip.lib.gh_abi_version() == 2  # entries were added, none changed meaning
    for k, name in enumerate(("OK", "TOO_FEW", "DEGENERATE", "INCONSISTENT", "LOW_PARALLAX", "SKIPPED")):
        assert re.search(r"#define GH_TRACK_%s %d\b" % (name, k), header)
        assert getattr(estimator, "TRACK_" + name) == k == getattr(tr, name)
    # GH_ERR_ARG without a context: nothing else is looked at, no device is needed
    assert hip.lib.gh_triangulate_tracks_dev(None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, None) == 1


def _case(name):
    a, e = tc.arrays(), tc.expected()
    p = tc.index(name)
    return e["status"][p], e["n_good"][p], e["results"][p], e["tracks"][p], e["point_xyz"][p]


def test_census_reaches_what_it_was_built_for():
    a, e = tc.arrays(), tc.expected()
    L = tr.LANES
    assert a["n_points"] == 33 and a["n_points"] % 32 != 0  # neither a wave (8 points) nor a workgroup (32) is full
    # track lengths on both sides of the group boundary, and many trips
    lengths = {name: len(e["tracks"][tc.index(name)]) for name in a["names"]}
    assert [lengths[n] for n in ("len0", "len1", "len2", "len7", "len8", "len9", "len16", "len17")] == [0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1]
    assert lengths["len600_drop1"] == tc.LONG == 75 * L
    for n in ("len2", "len7", "len8", "len9", "len16", "len17"):
        st, good, r, track, _ = _case(n)
        assert st == tr.OK and good == lengths[n] and r["drops"] == 0
    # interleaved, descending point order: consecutive observations belong to different points, and the order goes down
    pts = a["obs_point"][:40].astype(np.int64)
    assert (pts[1:] != pts[:-1]).all() and (np.diff(pts[:30]) < 0).sum() >= 25
    for p, track in enumerate(e["tracks"]):
        assert track == sorted(track)
        if len(track) > 1:
            assert max(np.diff(track)) > 1 or a["names"][p].startswith("len600")  # not stored as a block
    # indices out of range, both arrays, both sides
    assert {-1, tc.N_CAMS, tc.INT_MAX, tc.INT_MIN} <= set(a["obs_cam"].tolist())
    assert {-1, a["n_points"], tc.INT_MAX, tc.INT_MIN} <= set(a["obs_point"].tolist())
    assert _case("bad_cam_index")[:2] == (tr.OK, 3) and _case("bad_point_index")[:2] == (tr.OK, 2)
    bad = (a["obs_cam"] < 0) | (a["obs_cam"] >= tc.N_CAMS) | (a["obs_point"] < 0) | (a["obs_point"] >= a["n_points"])
    assert bad.sum() == 8 and not np.array(e["obs_good"])[bad].any()
    # masks
    assert (a["obs_use"] == 0).sum() == 3 and (a["point_select"] == 0).sum() == 2
    assert _case("masked_outliers")[:2] == (tr.OK, 3) and _case("masked_outliers")[2]["drops"] == 0
    assert _case("masked_too_few")[0] == tr.TOO_FEW and lengths["masked_too_few"] == 1
    for n in ("skipped", "skipped_empty"):
        st, good, r, track, X = _case(n)
        assert st == tr.SKIPPED and good == 0 and r is None and X == [tc.FILL_XYZ] * 3  # the point's values survive
    assert lengths["skipped"] == 4 and not any(e["obs_good"][i] for i in e["tracks"][tc.index("skipped")])
    # every status
    assert sorted(set(e["status"])) == [tr.OK, tr.TOO_FEW, tr.DEGENERATE, tr.INCONSISTENT, tr.LOW_PARALLAX, tr.SKIPPED]
    assert [_case(n)[0] for n in ("len0", "len1")] == [tr.TOO_FEW] * 2
    # drops of 0, 1 and 2; the outlier is what goes, also in a later trip and when both are ranks of one lane
    assert _case("drop1")[2]["dropped"] == [2] and _case("drop1")[:2] == (tr.OK, 5)
    assert sorted(_case("drop2")[2]["dropped"]) == [1, 5] and _case("drop2")[:2] == (tr.OK, 5)
    assert _case("len600_drop1")[2]["dropped"] == [300] and _case("len600_drop1")[:2] == (tr.OK, tc.LONG - 1)
    assert _case("outlier_rank7")[2]["dropped"] == [L - 1] and _case("outlier_rank8")[2]["dropped"] == [L]
    assert sorted(_case("two_in_one_lane")[2]["dropped"]) == [L, 2 * L] and _case("two_in_one_lane")[:2] == (tr.OK, 15)
    # a third outlier; the stop at min_views with drops to spare, with and without a drop
    st, _, r, _, X = _case("three_outliers")
    assert st == tr.INCONSISTENT and r["drops"] == tc.PARAMS["max_drops"] and X == [0.0] * 3
    st, _, r, _, _ = _case("two_skew_rays")
    assert st == tr.INCONSISTENT and r["drops"] == 0
    st, _, r, _, _ = _case("stop_at_min_views")
    assert st == tr.INCONSISTENT and r["drops"] == 1 < tc.PARAMS["max_drops"]
    # two +inf keys: the lower rank goes first
    st, good, r, track, X = _case("tie_behind")
    assert st == tr.OK and good == 3 and r["dropped"] == [0, 2] and r["anchor"] == 1
    cam, xy = a["cam_pose"].tolist(), a["obs_xy"].tolist()
    X_first = tr.solve(tr.total([(k, tr.normal_terms(tr.ray(cam[a["obs_cam"][i]], *xy[i]), cam[a["obs_cam"][i]][4:7]))
                                 for k, i in enumerate(track)]))
    keys = [tr.classify(cam[a["obs_cam"][i]], xy[i][0], xy[i][1], X_first, 0.004 ** 2)[1] for i in track]
    assert keys[0] == keys[2] == tr.INF and max(keys[1], keys[3], keys[4]) < 1e-20
    # NaNs, identical centres, parallax
    assert np.isnan(a["obs_xy"]).sum() == 1 and np.isnan(a["cam_pose"]).sum() == 2
    assert [_case(n)[0] for n in ("nan_xy", "nan_pose", "same_centre")] == [tr.DEGENERATE] * 3
    st, good, r, _, X = _case("nan_translation")  # regular pivots, a NaN point: two ties of +inf keys, then three clean rays
    assert st == tr.OK and good == 3 and r["dropped"] == [0, 1] and all(v == v for v in X)
    c = [a["obs_cam"][i] for i in _case("same_centre")[3]]
    assert len(set(c)) == 3 and len({tuple(cam[k]) for k in c}) == 1
    st, _, r, _, _ = _case("low_parallax")
    assert st == tr.LOW_PARALLAX and r["drops"] == 0
    # a dropped first observation moves the anchor: against rank 0 the parallax would have been wide
    st, _, r, track, _ = _case("anchor_dropped_low")
    assert st == tr.LOW_PARALLAX and r["dropped"] == [0] and r["anchor"] == 1
    d = [tr.ray(cam[a["obs_cam"][i]], *xy[i]) for i in track]
    assert sum(x * y for x, y in zip(d[0], d[1])) < tc.PARAMS["min_parallax_cos"] < sum(x * y for x, y in zip(d[1], d[2]))
    st, good, r, _, _ = _case("anchor_dropped_ok")
    assert st == tr.OK and good == 4 and r["dropped"] == [0] and r["anchor"] == 1
    # a duplicated observation, -0.0
    st, good, _, track, _ = _case("duplicate")
    assert st == tr.OK and good == 4
    assert a["obs_cam"][track[1]] == a["obs_cam"][track[3]] and a["obs_xy"][track[1]].tobytes() == a["obs_xy"][track[3]].tobytes()
    st, _, _, track, X = _case("neg_zero")
    assert st == tr.OK and a["obs_xy"][track[0]].tobytes() == np.array([-0.0, -0.0]).tobytes()
    assert np.signbit(a["cam_pose"][a["obs_cam"][track[0]], 4:6]).all()
    # obs_good: the final live observations of OK points, nothing else
    assert sum(e["obs_good"]) == sum(g for g, s in zip(e["n_good"], e["status"]) if s == tr.OK) > 700
    assert all(g == 0 for g, s in zip(e["n_good"], e["status"]) if s != tr.OK)


def test_permuted_arrays_keep_every_track():
    a = tc.arrays()
    b, perm = tc.permuted(a, seed=4)
    assert sorted(perm.tolist()) == list(range(len(perm))) and (perm != np.arange(len(perm))).sum() > 700
    e = tc.expected()
    eb = tr.tracks(b["cam_pose"].tolist(), b["obs_cam"].tolist(), b["obs_point"].tolist(), b["obs_xy"].tolist(), b["n_points"],
                   b["obs_use"].tolist(), b["point_select"].tolist(), [[tc.FILL_XYZ] * 3] * b["n_points"], **tc.PARAMS)
    for p in range(a["n_points"]):
        assert [perm[i] for i in eb["tracks"][p]] == e["tracks"][p]
    assert eb["status"] == e["status"] and eb["n_good"] == e["n_good"]
    assert np.array(eb["point_xyz"]).tobytes() == np.array(e["point_xyz"]).tobytes()
    assert [eb["obs_good"][i] for i in np.argsort(perm)] == e["obs_good"]


def test_restatement_recovers_ground_truth():
    """Exact observations of 2000 points from 40 cameras at ground truth, max_reproj 1e-9: every point OK without a drop.
    Measured: the largest distance from ground truth is 1.99e-14 (a numpy prototype of the algorithm gave 2.1e-14); bound 1e-9,
    since a sign or a transpose error is O(1)."""
    g, e = tc.graph(False), tc.graph_expected(False)
    assert e["status"] == [tr.OK] * 2000 and e["n_good"] == [6] * 2000
    assert all(r["drops"] == 0 for r in e["results"]) and sum(e["obs_good"]) == 12000
    err = np.linalg.norm(np.array(e["point_xyz"]) - g["point_xyz_gt"], axis=1).max()
    print("largest distance from ground truth: %.3e" % err)
    assert err <= 1e-9


def test_restatement_on_noisy_observations_with_outliers():
    """Noise 0.002, 5 % outliers (x50), max_reproj 0.01, max_drops 2.  Measured: 1994 / 2000 points OK (the other six
    INCONSISTENT); of the OK points 1456 / 486 / 52 went through 0 / 1 / 2 drops; the largest distance of an OK point from
    ground truth is 0.0746.  Bounds: at least 99 % OK, every OK point within 0.15 (twice the 0.075 a numpy prototype of the
    algorithm gave; a wrong point is O(1) away)."""
    g, e = tc.graph(True), tc.graph_expected(True)
    st = np.array(e["status"])
    ok = st == tr.OK
    drops = np.bincount([r["drops"] for r, s in zip(e["results"], st) if s == tr.OK], minlength=3)
    err = np.linalg.norm(np.array(e["point_xyz"]) - g["point_xyz_gt"], axis=1)
    print("OK %d / 2000, statuses %s, drops of OK points %s, largest distance %.4f" % (ok.sum(), np.bincount(st, minlength=6), drops, err[ok].max()))
    assert ok.sum() >= 1980
    assert err[ok].max() <= 0.15
    assert np.array(e["n_good"])[ok].min() >= 4 and drops[1] > 100 and drops[2] > 10  # the rounds are exercised
    assert np.array(e["obs_good"]).sum() == np.array(e["n_good"]).sum()


MIDPOINT_DEVIATION = 2.14e-13  # measured: the largest |X - midpoint| entry over the 200 pairs below


def test_two_observations_give_the_midpoint_of_the_common_perpendicular():
    """For two rays the least-squares point is the midpoint of their common perpendicular.  The formula below (closest
    points of two lines, numpy) shares nothing with the restatement.  Measured deviation 2.14e-13 on points 6 .. 9 units from
    cameras 10 units from the origin; asserted at 64 times that."""
    from gslam_amd.ba_synth import quat_to_R
    g = tc.graph(True)
    R, centre = quat_to_R(g["cam_pose"][:, :4]), g["cam_pose"][:, 4:]
    worst = 0.0
    for p in range(0, 2000, 10):
        pair = (6 * p, 6 * p + 3)
        r = tr.point([(g["cam_pose"][g["obs_cam"][i]].tolist(), *g["obs_xy"][i].tolist()) for i in pair], max_reproj=1e9)
        assert r["status"] == tr.OK
        (a, ca), (b, cb) = [(R[g["obs_cam"][i]] @ np.r_[g["obs_xy"][i], 1.0], centre[g["obs_cam"][i]]) for i in pair]
        w = ca - cb
        aa, bb, ab, aw, bw = a @ a, b @ b, a @ b, a @ w, b @ w
        den = aa * bb - ab * ab
        s, t = (ab * bw - bb * aw) / den, (aa * bw - ab * aw) / den
        mid = 0.5 * ((ca + s * a) + (cb + t * b))
        worst = max(worst, np.abs(np.array(r["X"]) - mid).max())
    print("largest deviation from the midpoint: %.3e" % worst)
    assert worst <= 64 * MIDPOINT_DEVIATION
