"""Map-point summaries: descriptor, view direction, range (gh_describe_points_dev).  Perf probe, not part of the product.

  map1   1000 frames x cap 2000, the last 100 new, each matched against 1 map frame (row 1 of tools/track_extend_probe.py)

The scene is the one of tools/track_extend_probe.py after a real gh_localize_pairs_dev -> gh_extend_tracks_dev ->
gh_triangulate_tracks_dev of the new points (outside the timed windows): the map as the extension leaves it, padding included
(n_obs = N, n_points = PC).  The descriptors are synthetic (random bytes: 64 MB), the octaves random in 0 .. 7, the poses the
scene's positions with the localised poses of the new frames.

Reported: the median of the whole call over all points (device-resident, ended by a synchronise) over 20 calls after a warm-up,
with the range; the same for the refresh of the points that the last 10 new frames see (point_select); from gh_prof_* in a run
of its own (event timing slows the host side) the parts of the full call; and, on the same machine in the same run, the route a
user had before this entry: download the descriptors, the keypoints, the observation arrays, the poses, the points and the
status, a vectorised numpy restatement of the contract, upload of the six per-point arrays (median of --host-repeats runs).
The host route's arrays are compared with the device's.  Prints one JSON object; --out FILE also writes it as text.

  python tools/point_describe_probe.py --out profiles/point_describe.txt"""
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
from gslam_amd import estimator, hip  # noqa: E402
from localize_probe import CAP, CONFIGS, INLIER_THRESHOLD, INTRINSICS, N_FRAMES, N_NEW, RANSAC_THRESHOLD, SEED, median, stats, synth_map  # noqa: E402
from track_extend_probe import MIN_VIEWS, add_new_pairs  # noqa: E402

PARTS = ("pdsc_keys", "pdsc_index", "pdsc_narrow", "pdsc_wide")
OUTPUTS = estimator.DESCRIBE_OUTPUTS
REFRESH_FRAMES = 10
SCALE, LEVELS, MAX_VIEWS = 1.2, 8, 64
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def host_describe(kps, desc, counts, poses, obs_cam, obs_point, obs_node, n_points, xyz, status):
    """The numpy restatement a user had to write (no obs_use, every point selected): the tracks grouped by length, each group
    vectorised; the direction in the contract's order of additions.  -> dict of arrays."""
    F, cap = N_FRAMES, CAP
    N = F * cap
    cnt = np.clip(counts.astype(np.int64), 0, cap)
    p, n = obs_point.astype(np.int64), obs_node.astype(np.int64)
    ok = (p >= 0) & (p < n_points) & (n >= 0) & (n < N)
    ns = np.where(ok, n, 0)
    ok &= (ns % cap < cnt[ns // cap]) & (obs_cam == ns // cap)
    ks = np.flatnonzero(ok)
    ks = ks[np.argsort(p[ks], kind="stable")]  # by point, ascending observation index inside a point
    ids, start, length = np.unique(p[ks], return_index=True, return_counts=True)
    usable = status == 0
    state = np.where(usable, 1, 2).astype(np.uint8)
    keep = usable[ids]
    ids, start, length = ids[keep], start[keep], length[keep]
    state[ids] = 0
    out = dict(point_state=state, point_desc=np.zeros((n_points, 32), np.uint8), point_obs=np.full((n_points, 2), -1, np.int32),
               point_views=np.zeros(n_points, np.int32), point_normal=np.zeros((n_points, 3)), point_dist=np.zeros((n_points, 2)))
    out["point_views"][ids] = length
    pw = np.ones(LEVELS)
    for l in range(1, LEVELS):
        pw[l] = pw[l - 1] * SCALE
    octave = kps[..., 5].copy().view(np.int32).reshape(-1)
    flat = desc.reshape(N, 32)
    for L in np.unique(length):
        g = np.flatnonzero(length == L)
        track = ks[start[g][:, None] + np.arange(L)[None, :]]              # n_g x L observation indices
        M = min(int(L), MAX_VIEWS)
        cand = track if L <= MAX_VIEWS else track[:, (np.arange(M, dtype=np.int64) * int(L)) // M]
        d = flat[n[cand]]                                                    # n_g x M x 32
        D = POPCOUNT[d[:, :, None, :] ^ d[:, None, :, :]].sum(3)             # n_g x M x M
        med = np.sort(D, axis=2)[:, :, (M - 1) // 2]
        best = np.argmin(med, axis=1)                                        # the first minimum
        rows = np.arange(len(g))
        chosen = cand[rows, best]
        out["point_desc"][ids[g]] = flat[n[chosen]]
        out["point_obs"][ids[g], 0] = chosen
        out["point_obs"][ids[g], 1] = track[:, 0]
        v = xyz[ids[g]][:, None, :] - poses[n[track] // cap, 4:]            # n_g x L x 3
        r2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        with np.errstate(all="ignore"):
            u = v * (1.0 / np.sqrt(r2))[..., None]
            s = np.zeros((len(g), 8, 3))
            for i in range(int(L)):
                s[:, i % 8] = s[:, i % 8] + u[:, i]
            total = ((s[:, 0] + s[:, 4]) + (s[:, 2] + s[:, 6])) + ((s[:, 1] + s[:, 5]) + (s[:, 3] + s[:, 7]))
            out["point_normal"][ids[g]] = total / float(L)
            level = np.clip(octave[n[track[:, 0]]], 0, LEVELS - 1)
            hi = np.sqrt(r2[:, 0]) * pw[level]
            out["point_dist"][ids[g], 0] = hi / pw[LEVELS - 1]
            out["point_dist"][ids[g], 1] = hi
    for k in ("point_normal", "point_dist"):
        out[k][np.isnan(out[k])] = np.float64("nan")
    n_ok = len(ids)
    out["totals"] = np.array([n_ok, int((state == 1).sum()), int((state == 2).sum()), int((length > MAX_VIEWS).sum())], np.int32)
    return out


def measure(ctx, name, repeats, host_repeats):
    import torch
    s = add_new_pairs(synth_map(CONFIGS[name]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    rng = np.random.default_rng(5)
    kps_host = s["kps"].copy()
    kps_host[..., 5] = rng.integers(0, LEVELS, (N_FRAMES, CAP)).astype(np.int32).view(np.float32)
    d["kps"] = dev(kps_host)
    desc = dev(rng.integers(0, 256, (N_FRAMES, CAP, 32), dtype=np.uint8))
    n_map, P = len(s["point_xyz"]), len(s["pair_q"])
    n_loc = P - (N_NEW - 1)  # the localisation sees the new-versus-map pairs only
    loc = estimator.localize_pairs(ctx, d["kps"], d["counts"], d["pair_q"][:n_loc].contiguous(), d["pair_t"][:n_loc].contiguous(),
                                   d["idx1"][:n_loc].contiguous(), d["keep"][:n_loc].contiguous(), d["node_point"], d["point_xyz"],
                                   d["status"], INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    ext = estimator.extend_tracks(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["keep"], d["node_point"], n_map,
                                  loc["row_point"], loc["row_inlier"], INTRINSICS, MIN_VIEWS)
    N = N_FRAMES * CAP
    PC = n_map + N // 2
    first_new = N_FRAMES - N_NEW
    poses_host = np.zeros((N_FRAMES, 7))
    poses_host[:, 3] = 1.0
    poses_host[:, 4:] = s["positions"]
    poses = dev(poses_host)
    poses[first_new:] = loc["poses"][first_new:]
    xyz = torch.zeros((PC, 3), dtype=torch.float64, device="cuda")
    xyz[:n_map] = d["point_xyz"]
    tri = estimator.triangulate_tracks(ctx, poses, ext["obs_cam"], ext["obs_point"], ext["obs_xy"], PC, point_select=ext["point_new"],
                                       point_xyz=xyz)
    status = torch.full((PC,), estimator.TRACK_TOO_FEW, dtype=torch.int32, device="cuda")
    status[:n_map] = d["status"]
    status = torch.where(ext["point_new"] != 0, tri["status"], status)
    recent = (ext["obs_cam"] >= N_FRAMES - REFRESH_FRAMES) & (ext["obs_point"] >= 0)
    select = torch.zeros(PC, dtype=torch.uint8, device="cuda")
    select[ext["obs_point"][recent].long()] = 1
    # (allocations and the scratch's growth outside the timed windows)
    out = estimator.describe_points(ctx, d["kps"], desc, d["counts"], poses, ext["obs_cam"], ext["obs_point"], ext["obs_node"], PC, xyz,
                                    point_status=status)
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    prm = estimator.point_desc_default_params()
    assert (prm.scale_factor, prm.n_levels, prm.max_views) == (SCALE, LEVELS, MAX_VIEWS)

    def describe(sel=None, into=out):
        ctx.check(hip.lib.gh_describe_points_dev(ctx.h, pv(d["kps"]), pv(desc), pv(d["counts"]), N_FRAMES, CAP, pv(poses), pv(ext["obs_cam"]),
                                                 pv(ext["obs_point"]), pv(ext["obs_node"]), None, N, PC, pv(xyz), pv(status), pv(sel),
                                                 C.byref(prm), *(pv(into[k]) for k in OUTPUTS)))
        torch.cuda.synchronize()

    full_us = median(describe, repeats, 5)
    full = {k: out[k].cpu().numpy() for k in OUTPUTS}
    scratch = {k: out[k].clone() for k in OUTPUTS}
    refresh_us = median(lambda: describe(select, scratch), repeats, 5)
    refresh_totals = scratch["totals"].cpu().numpy().tolist()
    ctx.prof_enable(True)
    for _ in range(repeats):
        describe()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}

    t_host, t_down, h = [], [], None
    for rep in range(host_repeats + 1):
        t0 = time.perf_counter()
        a = [t.cpu().numpy() for t in (d["kps"], desc, d["counts"], poses, ext["obs_cam"], ext["obs_point"], ext["obs_node"])]
        x, st = xyz.cpu().numpy(), status.cpu().numpy()
        t1 = time.perf_counter()
        h = host_describe(*a, PC, x, st)
        up = [dev(h[k]) for k in OUTPUTS if k != "totals"]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:  # (the first run warms the allocator)
            t_down.append(t1 - t0)
            t_host.append(t2 - t0)
        del up
    same = {k: bool(h[k].tobytes() == full[k].tobytes()) for k in OUTPUTS}
    views = full["point_views"]
    return {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "new_frames": N_NEW, "nodes": N,
            "observations_in_use": int(ext["totals"].cpu().numpy()[0]), "point_capacity": PC,
            "totals_ok_empty_not_ok_sampled": full["totals"].tolist(), "views_max": int(views.max()),
            "views_mean_of_ok": round(float(views[views > 0].mean()), 2), "describe_us": full_us, "describe_parts_us": parts,
            "parts_sum_us": round(sum(parts.values()), 1), "refresh_frames": REFRESH_FRAMES, "refresh_points_selected": int(select.sum().item()),
            "refresh_totals_ok_empty_not_ok_sampled": refresh_totals, "refresh_us": refresh_us, "host_download_us": stats(t_down),
            "host_route_us": stats(t_host), "host_route_over_describe": round(float(np.median(t_host)) * 1e6 / full_us["median"], 1),
            "host_route_gives_the_same_arrays": all(same.values()), "host_route_same_by_array": same}


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
            f.write("tools/point_describe_probe.py: map-point summaries (descriptor, view direction, range), gh_describe_points_dev "
                    "(synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
