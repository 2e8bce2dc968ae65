"""The local window of the new frames for bundle adjustment (gh_ba_window_dev).  Perf probe, not part of the product.

  map1   1000 frames x cap 2000; the last 100 frames are new and were matched against 1 map frame each; the last 10 are the seeds

The arrays come from a real extension, as tools/track_extend_probe.py builds them: the scene of tools/localize_probe.py with
chains of new tracks among the new frames, gh_localize_pairs_dev, gh_extend_tracks_dev, then gh_triangulate_tracks_dev of the new
points at the poses the localisation found -- all outside the timed windows.  The window then takes obs_cam, obs_point, obs_xy
at their capacity N = 2 M and the points at PC = n_points + N / 2; point_use is status == OK merged over the map and the new
triangulation, obs_use is obs_good of that triangulation for the observations of new points and 1 for those of map points (the
synthetic map has no earlier triangulation: the map and the localisation vouch for them); both merged on the device with torch.

Two routes to the same place, the host arrays gh_ba_solve takes:
  (a) gh_ba_window_dev, the download of the 32 bytes of totals and of the compact prefixes (ba.window_problem);
  (b) what a user had before this entry, on the same machine in the same run: download the padded obs_cam, obs_point, obs_xy,
      the use bytes, the seeds, and the poses and points the problem is cut from; a vectorised numpy restatement of the rules.
Their arrays must be equal.  Medians of 20 calls after a warm-up, with the range; the parts from gh_prof_* in a run of their
own (event timing slows the host side); the same call on the arrays cut to their totals (no padding) beside it.  Prints one
JSON object; --out FILE also writes it as text.

  python tools/ba_window_probe.py --out profiles/ba_window.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gslam_amd import ba, estimator, hip  # noqa: E402
from localize_probe import CAP, CONFIGS, INLIER_THRESHOLD, INTRINSICS, N_FRAMES, N_NEW, RANSAC_THRESHOLD, SEED, median, stats, synth_map  # noqa: E402
from track_extend_probe import MIN_VIEWS, add_new_pairs  # noqa: E402

PARTS = ("baw_count", "baw_seen", "baw_shared", "baw_local", "baw_points", "baw_fixed", "baw_flags", "baw_scan", "baw_emit")
N_SEEDS, MIN_SHARED, MIN_POINT_OBS = 10, 15, 2
PROBLEM = ("cam_pose", "cam_dof", "point_xyz", "obs_cam", "obs_point", "obs_xy", "win_cam", "win_point")


def host_window(cam_pose, point_xyz, obs_cam, obs_point, obs_xy, obs_use, point_use, cam_seed, min_shared, min_point_obs):
    """The numpy restatement a user had to write -> the dict gh_ba_solve takes, with win_cam, win_point and the totals."""
    nc, npts = len(cam_pose), len(point_xyz)
    cam, pt = obs_cam.astype(np.int64), obs_point.astype(np.int64)
    ok = (obs_use != 0) & (cam >= 0) & (cam < nc) & (pt >= 0) & (pt < npts)
    cam, pt = np.where(ok, cam, 0), np.where(ok, pt, 0)
    ok &= point_use[pt] != 0
    live = ok & (np.bincount(pt[ok], minlength=npts) >= min_point_obs)[pt]
    seed = cam_seed != 0
    seen = np.zeros(npts, bool)
    seen[pt[live & seed[cam]]] = True
    shared = np.bincount(cam[live & seen[pt]], minlength=nc)
    local = (seed & (shared >= 1)) | (shared >= max(min_shared, 1))
    wpt = np.zeros(npts, bool)
    wpt[pt[live & local[cam]]] = True
    src = np.flatnonzero(ok & wpt[pt])
    in_cam = local.copy()
    in_cam[cam[src]] = True
    cam_slot, point_slot = np.cumsum(in_cam) - 1, np.cumsum(wpt) - 1
    cams, points = np.flatnonzero(in_cam), np.flatnonzero(wpt)
    return {"cam_pose": cam_pose[cams], "cam_dof": np.where(local[cams], 63, 0).astype(np.int32), "point_xyz": point_xyz[points],
            "obs_cam": cam_slot[cam[src]].astype(np.int32), "obs_point": point_slot[pt[src]].astype(np.int32), "obs_xy": obs_xy[src],
            "win_cam": cams.astype(np.int32), "win_point": points.astype(np.int32),
            "totals": [len(cams), int(local.sum()), len(cams) - int(local.sum()), 0, len(points), len(src), int((in_cam & seed).sum()),
                       int(ok.sum())]}


def build_map(ctx, name):
    """localize -> extend -> triangulate the new points: the device arrays of the extended map and the use bytes."""
    import torch
    s = add_new_pairs(synth_map(CONFIGS[name]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    n_points, P = len(s["point_xyz"]), len(s["pair_q"])
    n_loc = P - (N_NEW - 1)
    loc = estimator.localize_pairs(ctx, d["kps"], d["counts"], d["pair_q"][:n_loc].contiguous(), d["pair_t"][:n_loc].contiguous(),
                                   d["idx1"][:n_loc].contiguous(), d["keep"][:n_loc].contiguous(), d["node_point"], d["point_xyz"],
                                   d["status"], INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    ext = estimator.extend_tracks(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["keep"], d["node_point"], n_points,
                                  loc["row_point"], loc["row_inlier"], INTRINSICS, MIN_VIEWS)
    N = N_FRAMES * CAP
    PC = n_points + N // 2
    poses = np.zeros((N_FRAMES, 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = s["positions"]
    poses = dev(poses)
    poses[N_FRAMES - N_NEW:] = loc["poses"][N_FRAMES - N_NEW:]
    xyz = torch.zeros((PC, 3), dtype=torch.float64, device="cuda")
    xyz[:n_points] = d["point_xyz"]
    tri = estimator.triangulate_tracks(ctx, poses, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], PC, point_select=ext["point_new"],
                                       point_xyz=xyz)
    point_use = tri["status"] == estimator.TRACK_OK
    point_use[:n_points] = d["status"] == estimator.TRACK_OK
    of_map_point = (ext["obs_point"] >= 0) & (ext["obs_point"] < n_points)
    obs_use = ((tri["obs_good"] != 0) | of_map_point).to(torch.uint8).contiguous()
    cam_seed = torch.zeros(N_FRAMES, dtype=torch.uint8, device="cuda")
    cam_seed[N_FRAMES - N_SEEDS:] = 1
    torch.cuda.synchronize()
    ext_totals = ext["totals"].cpu().numpy().tolist()
    return dict(cam_pose=poses, point_xyz=tri["point_xyz"], obs_cam=ext["obs_cam"], obs_point=ext["obs_point"], obs_xy=ext["obs_xy"],
                obs_use=obs_use, point_use=point_use.to(torch.uint8).contiguous(), cam_seed=cam_seed, map_points=n_points,
                n_obs=ext_totals[0], n_points_total=ext_totals[1], points_ok=int(point_use.sum().item()),
                obs_used=int(obs_use.sum().item()))


def measure(ctx, name, repeats, host_repeats):
    import torch
    m = build_map(ctx, name)
    inputs = ("cam_pose", "point_xyz", "obs_cam", "obs_point", "obs_xy", "obs_use", "point_use", "cam_seed")
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    par = hip.BaWindowParams(MIN_SHARED, MIN_POINT_OBS)

    def entry(arrays):
        """-> (the call on preallocated outputs, its outputs); allocations and the scratch's growth stay outside the timed windows"""
        win = ba.window(ctx, *(arrays[k] for k in inputs[:5]), arrays["cam_seed"], obs_use=arrays["obs_use"], point_use=arrays["point_use"],
                        min_shared=MIN_SHARED, min_point_obs=MIN_POINT_OBS)
        nc, npts, no = arrays["cam_pose"].shape[0], arrays["point_xyz"].shape[0], arrays["obs_cam"].numel()
        args = [ctx.h, nc, npts, no] + [pv(arrays[k]) for k in inputs] + [None, C.byref(par)] + [pv(win[k]) for k in ba.WINDOW_OUTPUTS]
        return (lambda: ctx.check(hip.lib.gh_ba_window_dev(*args))), win

    call, win = entry(m)

    def device_only():
        call()
        torch.cuda.synchronize()

    problem = [None]

    def route_a():
        call()
        problem[0] = ba.window_problem(win)

    window_us = median(device_only, repeats, 5)
    route_a_us = median(route_a, repeats, 5)
    ctx.prof_enable(True)
    for _ in range(repeats):
        device_only()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}

    # the same call without the padding: the arrays cut to their totals
    cut = dict(m, obs_cam=m["obs_cam"][:m["n_obs"]].contiguous(), obs_point=m["obs_point"][:m["n_obs"]].contiguous(),
               obs_xy=m["obs_xy"][:m["n_obs"]].contiguous(), obs_use=m["obs_use"][:m["n_obs"]].contiguous(),
               point_xyz=m["point_xyz"][:m["n_points_total"]].contiguous(), point_use=m["point_use"][:m["n_points_total"]].contiguous())
    call_cut, win_cut = entry(cut)

    def device_cut():
        call_cut()
        torch.cuda.synchronize()

    cut_us = median(device_cut, repeats, 5)
    same_cut = bool(torch.equal(win_cut["totals"], win["totals"]))

    t_host, t_down, h = [], [], None
    for rep in range(host_repeats + 1):
        t0 = time.perf_counter()
        host = {k: m[k].cpu().numpy() for k in inputs}
        t1 = time.perf_counter()
        h = host_window(*(host[k] for k in inputs), MIN_SHARED, MIN_POINT_OBS)
        t2 = time.perf_counter()
        if rep:  # (the first run warms the allocator)
            t_down.append(t1 - t0)
            t_host.append(t2 - t0)
    p = problem[0]
    same = bool(h["totals"] == p["totals"] and all(np.ascontiguousarray(h[k]).tobytes() == p[k].tobytes() for k in PROBLEM))
    total_parts = sum(parts.values())
    prefix_bytes = sum(p[k].nbytes for k in PROBLEM) + p["win_obs_src"].nbytes + 32
    padded_bytes = sum(m[k].numel() * m[k].element_size() for k in inputs)
    return {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "new_frames": N_NEW, "seeds": N_SEEDS,
            "min_shared": MIN_SHARED, "capacity_cams_points_obs": [N_FRAMES, int(m["point_xyz"].shape[0]), N_FRAMES * CAP],
            "map_obs_points_points_ok_obs_used": [m["n_obs"], m["n_points_total"], m["points_ok"], m["obs_used"]],
            "totals_cams_local_fixed_held_points_obs_seeds_usable": p["totals"],
            "window_us": window_us, "route_a_window_and_download_us": route_a_us, "downloaded_bytes": prefix_bytes,
            "window_parts_us": parts, "parts_sum_us": round(total_parts, 1),
            "scan_share_of_parts": round(parts.get("baw_scan", 0.0) / total_parts, 3) if total_parts else None,
            "window_without_padding_us": cut_us, "without_padding_gives_the_same_totals": same_cut,
            "padding_share_of_call": round(1.0 - cut_us["median"] / window_us["median"], 3),
            "host_download_us": stats(t_down), "host_downloaded_bytes": padded_bytes, "route_b_download_and_numpy_us": stats(t_host),
            "route_b_over_route_a": round(float(np.median(t_host)) * 1e6 / route_a_us["median"], 1),
            "host_route_gives_the_same_arrays": same}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="map1")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    results = []
    for name in a.configs.split(","):
        results.append(measure(ctx, name, a.repeats, a.host_repeats))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/ba_window_probe.py: the local window of the new frames, gh_ba_window_dev (synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
