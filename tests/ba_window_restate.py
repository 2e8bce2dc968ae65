"""gh_ba_window_dev and gh_ba_window_scatter_dev restated in plain Python on lists, dicts and sets: the rules of
include/gslam_hip.h in their order, one loop per rule, no numpy and nothing clever.  tests/test_ba_window_cpu.py holds it to
an independent vectorised brute force; tests/test_ba_window_gpu.py holds the device to it byte for byte."""

WIN_NONE, WIN_LOCAL, WIN_FIXED = 0, 1, 2
KF_SE3 = 63


def window(n_cams, n_points, cam_pose, point_xyz, obs_cam, obs_point, obs_xy, cam_seed, obs_use=None, point_use=None, cam_hold=None,
           min_shared=15, min_point_obs=2):
    """cam_pose: n_cams rows of 7, point_xyz: n_points rows of 3, obs_xy: n_obs rows of 2, the rest flat lists.  -> dict of lists
    at the capacities of the device's outputs, plus the sets behind them (`usable`, `live_points`, `seen`, `window_points`)."""
    n_obs = len(obs_cam)
    # USABLE
    usable = []
    for k in range(n_obs):
        if obs_use is not None and obs_use[k] == 0:
            continue
        c, p = obs_cam[k], obs_point[k]
        if not (0 <= c < n_cams) or not (0 <= p < n_points):
            continue
        if point_use is not None and point_use[p] == 0:
            continue
        usable.append(k)
    # n_use, LIVE
    n_use = {}
    for k in usable:
        n_use[obs_point[k]] = n_use.get(obs_point[k], 0) + 1
    live_points = {p for p, n in n_use.items() if n >= min_point_obs}
    live = [k for k in usable if obs_point[k] in live_points]
    # SEEN
    seen = {obs_point[k] for k in live if cam_seed[obs_cam[k]] != 0}
    # shared
    shared = [0] * n_cams
    for k in live:
        if obs_point[k] in seen:
            shared[obs_cam[k]] += 1
    # LOCAL
    local = {c for c in range(n_cams) if (cam_seed[c] != 0 and shared[c] >= 1) or shared[c] >= max(min_shared, 1)}
    # window points and window observations
    window_points = {obs_point[k] for k in live if obs_cam[k] in local}
    win_obs = [k for k in usable if obs_point[k] in window_points]
    # FIXED
    fixed = {obs_cam[k] for k in win_obs} - local
    # numbering
    cams = sorted(local | fixed)
    points = sorted(window_points)
    cam_slot = [-1] * n_cams
    for i, c in enumerate(cams):
        cam_slot[c] = i
    point_slot = [-1] * n_points
    for j, p in enumerate(points):
        point_slot[p] = j
    held = {c for c in local if cam_hold is not None and cam_hold[c] != 0}

    pad_c, pad_p, pad_o = n_cams - len(cams), n_points - len(points), n_obs - len(win_obs)
    out = dict(
        cam_class=[WIN_LOCAL if c in local else (WIN_FIXED if c in fixed else WIN_NONE) for c in range(n_cams)],
        cam_shared=shared, cam_slot=cam_slot, point_slot=point_slot,
        win_cam=cams + [-1] * pad_c,
        win_cam_dof=[KF_SE3 if (c in local and c not in held) else 0 for c in cams] + [0] * pad_c,
        win_cam_pose=[list(cam_pose[c]) for c in cams] + [[0.0] * 7 for _ in range(pad_c)],
        win_point=points + [-1] * pad_p,
        win_point_xyz=[list(point_xyz[p]) for p in points] + [[0.0] * 3 for _ in range(pad_p)],
        win_obs_cam=[cam_slot[obs_cam[k]] for k in win_obs] + [-1] * pad_o,
        win_obs_point=[point_slot[obs_point[k]] for k in win_obs] + [-1] * pad_o,
        win_obs_src=win_obs + [-1] * pad_o,
        win_obs_xy=[list(obs_xy[k]) for k in win_obs] + [[0.0, 0.0] for _ in range(pad_o)],
        totals=[len(cams), len(local), len(fixed), len(held), len(points), len(win_obs),
                len([c for c in cams if cam_seed[c] != 0]), len(usable)],
    )
    out.update(usable=set(usable), n_use=n_use, live_points=live_points, seen=seen, window_points=window_points)
    return out


def scatter(win_cam, win_cam_dof, n_win_cams, cam_pose_win, win_point, n_win_points, point_xyz_win, cam_pose, point_xyz):
    """-> (cam_pose, point_xyz) after gh_ba_window_scatter_dev, as new lists of rows."""
    cam_pose = [list(r) for r in cam_pose]
    point_xyz = [list(r) for r in point_xyz]
    for i in range(n_win_cams):
        if win_cam_dof[i] != 0 and 0 <= win_cam[i] < len(cam_pose):
            cam_pose[win_cam[i]] = list(cam_pose_win[i])
    for j in range(n_win_points):
        if 0 <= win_point[j] < len(point_xyz):
            point_xyz[win_point[j]] = list(point_xyz_win[j])
    return cam_pose, point_xyz
