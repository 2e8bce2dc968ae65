"""The specification of gh_ba_window_dev, pinned without a GPU: the plain-Python restatement (tests/ba_window_restate.py) against
an independent vectorised numpy brute force (incidence matrices, no loops over observations) on the census, the boundary soups,
the hub, the trajectory and 50 random cases; the figures the trajectory was chosen for; and every rule of the census shown in
the restatement's output by the name of the row that is there for it.  These tests pass without the device code: they pin what
tests/test_ba_window_gpu.py holds the device to."""
import numpy as np
import pytest

import ba_window_cases as wc
import ba_window_restate as rs


def brute(c, use_obs_use=True, use_point_use=True, use_hold=True, min_shared=None, min_point_obs=None):
    """The contract from camera x point incidence counts -> the outputs cut to their totals."""
    nc, npts = c["n_cams"], c["n_points"]
    ms = c["min_shared"] if min_shared is None else min_shared
    mp = c["min_point_obs"] if min_point_obs is None else min_point_obs
    cam, pt = c["obs_cam"].astype(np.int64), c["obs_point"].astype(np.int64)
    ok = (cam >= 0) & (cam < nc) & (pt >= 0) & (pt < npts)
    if use_obs_use:
        ok &= c["obs_use"] != 0
    if use_point_use:
        ok &= c["point_use"][np.where(ok, pt, 0)] != 0
    A = np.zeros((nc, npts), np.int64)                   # usable observations per (camera, point)
    np.add.at(A, (cam[ok], pt[ok]), 1)
    live = A.sum(0) >= mp
    L = A * live[None, :]
    seed = c["cam_seed"] != 0
    seen = L[seed].sum(0) > 0
    shared = (L * seen[None, :]).sum(1)
    local = (seed & (shared >= 1)) | (shared >= max(ms, 1))
    wpt = L[local].sum(0) > 0
    W = A * wpt[None, :]
    fixed = ~local & (W.sum(1) > 0)
    in_cam = local | fixed
    cam_slot = np.where(in_cam, np.cumsum(in_cam) - 1, -1)
    point_slot = np.where(wpt, np.cumsum(wpt) - 1, -1)
    src = np.flatnonzero(ok & wpt[np.where(ok, pt, 0)])
    hold = (c["cam_hold"] != 0) if use_hold else np.zeros(nc, bool)
    cams = np.flatnonzero(in_cam)
    return dict(cam_class=np.where(local, 1, np.where(fixed, 2, 0)), cam_shared=shared, cam_slot=cam_slot, point_slot=point_slot,
                win_cam=cams, win_cam_dof=np.where(local[cams] & ~hold[cams], 63, 0), win_cam_pose=c["cam_pose"][cams],
                win_point=np.flatnonzero(wpt), win_point_xyz=c["point_xyz"][wpt], win_obs_cam=cam_slot[cam[src]],
                win_obs_point=point_slot[pt[src]], win_obs_src=src, win_obs_xy=c["obs_xy"][src],
                totals=[int(in_cam.sum()), int(local.sum()), int(fixed.sum()), int((local & hold).sum()), int(wpt.sum()), len(src),
                        int((in_cam & seed).sum()), int(ok.sum())])


def _assert_agree(c, **kw):
    e, b = wc.as_arrays(wc.restate(c, **kw)), brute(c, **kw)
    t = b["totals"]
    assert e["totals"].tolist() == t, (c["name"], kw)
    nc, npts, no = c["n_cams"], c["n_points"], len(c["obs_cam"])
    for k in ("cam_class", "cam_shared", "cam_slot", "point_slot"):
        assert e[k].tolist() == b[k].tolist(), (c["name"], k, kw)
    for k, n, cap, width, pad in (("win_cam", t[0], nc, 1, -1), ("win_cam_dof", t[0], nc, 1, 0), ("win_cam_pose", t[0], nc, 7, 0.0),
                                  ("win_point", t[4], npts, 1, -1), ("win_point_xyz", t[4], npts, 3, 0.0), ("win_obs_cam", t[5], no, 1, -1),
                                  ("win_obs_point", t[5], no, 1, -1), ("win_obs_src", t[5], no, 1, -1), ("win_obs_xy", t[5], no, 2, 0.0)):
        assert len(e[k]) == cap * width, (c["name"], k)
        assert e[k][:n * width].tobytes() == np.ascontiguousarray(b[k]).astype(wc.DTYPE[k]).tobytes(), (c["name"], k, kw)
        assert (e[k][n * width:] == pad).all(), (c["name"], k, "padding")
    return t


VARIANTS = [dict(), dict(use_obs_use=False), dict(use_point_use=False), dict(use_hold=False), dict(min_shared=0), dict(min_shared=1),
            dict(min_point_obs=1), dict(min_point_obs=3)]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "as_given")
def test_census_restatement_equals_the_brute_force(kw):
    _assert_agree(wc.census(), **kw)


def test_census_figures():
    assert len(wc.CENSUS_ROWS) == 34 and len(set(wc.census()["rows"])) == 34
    assert _assert_agree(wc.census()) == [6, 4, 2, 2, 6, 18, 2, 24]


def test_every_rule_of_the_census_shows_in_the_restatement_by_name():
    c = wc.census()
    e = wc.restate(c)
    row = {name: k for k, name in enumerate(c["rows"])}
    # USABLE: the four indices out of range (and the two extreme ones), obs_use 0, point_use 0
    for name in ("bad_cam_minus1", "bad_cam_n", "bad_point_minus1", "bad_point_n", "bad_cam_int_max", "bad_point_int_min", "seed5_p0_unused",
                 "seed7_p7_unused", "seed7_p8_point_unused", "seed6_p8_point_unused"):
        assert row[name] not in e["usable"], name
    assert len(e["usable"]) == 24 == e["totals"][7]
    # n_use counts a pair given twice twice; min_point_obs - 1 and min_point_obs exactly
    assert e["n_use"][1] == 5 and e["n_use"][6] == 2 and e["n_use"][7] == c["min_point_obs"] - 1 and e["n_use"][4] == c["min_point_obs"]
    assert 7 not in e["live_points"] and 9 not in e["live_points"] and 8 not in e["n_use"] and {4, 6} <= e["live_points"]
    assert e["seen"] == {0, 1, 2, 3}
    assert e["cam_shared"] == [0, 0, 2, 3, 3, 0, 2, 4]
    L, F, N = rs.WIN_LOCAL, rs.WIN_FIXED, rs.WIN_NONE
    # 5: a seed without a live observation; 4: shared == min_shared (through the pair given twice); 2: min_shared - 1, sees window
    # points; 1: sees only points outside the window; 6: a seed below min_shared
    assert e["cam_class"] == [F, N, F, L, L, N, L, L] and e["cam_shared"][4] == c["min_shared"] and e["cam_shared"][2] == c["min_shared"] - 1
    assert e["window_points"] == {0, 1, 2, 3, 4, 10}
    assert 5 in e["live_points"] and 6 in e["live_points"]          # live, yet outside: 6 is seen only by the NONE camera 1
    for name in ("cam1_p5", "cam0_p5", "cam1_p6_first", "cam1_p6_again", "seed5_p7_short", "seed7_p9_single"):
        assert row[name] not in e["win_obs_src"], name
    for name in ("cam4_p1_first", "cam4_p1_again", "cam0_p4", "cam2_p10"):
        assert row[name] in e["win_obs_src"], name
    assert e["win_obs_src"][:18] == sorted(e["win_obs_src"][:18]) and e["win_obs_src"][18:] == [-1] * 16
    # numbering and dof: 0 FIXED and held, 2 FIXED, 3 LOCAL and held, 4 LOCAL, 6 a held seed, 7 a seed
    assert e["win_cam"] == [0, 2, 3, 4, 6, 7, -1, -1] and e["win_cam_dof"] == [0, 0, 0, 63, 0, 63, 0, 0]
    assert e["cam_slot"] == [0, -1, 1, 2, 3, -1, 4, 5] and e["win_point"][:7] == [0, 1, 2, 3, 4, 10, -1]
    assert e["totals"] == [6, 4, 2, 2, 6, 18, 2, 24]
    assert wc.restate(c, use_hold=False)["win_cam_dof"] == [0, 0, 63, 63, 63, 63, 0, 0]
    # without the use bytes camera 5 has a live observation of the SEEN point 0 and is LOCAL; point 8 enters
    assert wc.restate(c, use_obs_use=False)["cam_class"][5] == L and 8 in wc.restate(c, use_point_use=False)["window_points"]


def test_boundaries_and_hub():
    shapes, with_none = [], 0
    for c in wc.boundaries():
        t = _assert_agree(c)
        shapes.append((c["n_cams"], c["n_points"], len(c["obs_cam"])))
        assert t[1] >= 4 and t[2] >= 1 and 0 < t[4] < c["n_points"] and 0 < t[5] < t[7] < len(c["obs_cam"]), (c["name"], t)
        with_none += t[0] < c["n_cams"]
        e = wc.as_arrays(wc.restate(c))
        assert e["win_obs_src"][0] == 0 and e["win_obs_src"][t[5] - 1] == len(c["obs_cam"]) - 1  # the first and the last lane emit
        _assert_agree(c, use_obs_use=False, use_point_use=False, use_hold=False)
    assert with_none >= 4
    assert shapes == [(40, 100, 512), (40, 100, 513), (256, 90, 1500), (257, 90, 1500), (40, 512, 1500), (40, 513, 1500)]
    for order in ("frame_major", "track_major"):
        c = wc.hub(order)
        assert _assert_agree(c) == [257, 185, 72, 2, 3001, 6257, 1, 6257]
        e = wc.restate(c)
        assert e["n_use"][0] == 257 and e["cam_shared"][256] == 3001 and e["cam_shared"][:256] == [12] + [13] * 184 + [12] * 71


@pytest.mark.parametrize("min_shared", [15, 1])
def test_trajectory_figures(min_shared):
    c = wc.trajectory(min_shared)
    assert len(c["obs_cam"]) == 6000
    t = _assert_agree(c)
    assert (t[1], t[2], t[4], t[5]) == wc.TRAJECTORY_FIGURES[min_shared]
    assert t[6] == 2 and t[3] == 0 and t[7] == 6000
    assert wc.restate(c)["cam_shared"][50] == 2


def test_trajectory_in_three_orders():
    c = wc.trajectory(15)
    first = None
    for order in ("forward", "reversed", "shuffled"):
        d, perm = wc.reorder(c, order, seed=5)
        a = wc.as_arrays(wc.restate(d))
        got = ([a[k].tobytes() for k in wc.OUTPUTS if k not in wc.OBS_OUTPUTS], wc.in_source_order(a, perm))
        first = first or got
        assert got == first, order


def test_fifty_random_cases():
    rng = np.random.default_rng(77)
    reached = np.zeros(3, np.int64)
    for i in range(50):
        nc, npts, no = int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(0, 300))
        c = wc.soup(nc + 3, npts + 1, no + 4, seed=1000 + i, min_shared=int(rng.integers(0, 5)))
        t = _assert_agree(c, min_point_obs=int(rng.integers(1, 4)))
        reached += [t[1] > 0, t[2] > 0, t[0] < c["n_cams"]]
    assert (reached >= 10).all(), reached


def test_scatter_restatement():
    pose = [[float(10 * c + j) for j in range(7)] for c in range(4)]
    xyz = [[float(100 * p + j) for j in range(3)] for p in range(5)]
    new_pose = [[-1.0] * 7, [-2.0] * 7, [-3.0] * 7, [-4.0] * 7]
    new_xyz = [[-5.0] * 3, [-6.0] * 3, [-7.0] * 3]
    p2, x2 = rs.scatter([2, 0, 4, 3], [63, 0, 63, 63], 3, new_pose, [4, -1, 1], 2, new_xyz, pose, xyz)
    assert p2 == [pose[0], pose[1], new_pose[0], pose[3]]         # dof 0, out of range and past n_win_cams keep their rows
    assert x2 == [xyz[0], xyz[1], xyz[2], xyz[3], new_xyz[0]]
