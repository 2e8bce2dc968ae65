"""Extending the map with newly registered frames (gh_extend_tracks_dev).  Perf probe, not part of the product.

  map1 / map2 / map3   1000 frames x cap 2000; each of the last 100 frames matched against 1 / 2 / 3 map frames

The scene is the one of tools/localize_probe.py (geometrically consistent, so that gh_localize_pairs_dev produces real row_point /
row_inlier arrays: they are taken from a call of it, outside the timed windows), with one addition that gives the new tracks
something to do: every new frame is also paired with the next new frame, and 400 of its rows that no map frame answered are
matched one to one to such rows of the next frame -- chains of new tracks through the 100 new frames.  node_point is dirty in the
new frames, as the localisation leaves it.

Per configuration: the median of the whole call (device-resident, ended by a synchronise) over 20 calls after a warm-up, with
the range; from gh_prof_* in a run of its own (event timing slows the host side) the parts; and, on the same machine in the
same run, the route a user had before this entry: download node_point, row_point, row_inlier, idx1 and the inlier bytes, a
vectorised numpy / scipy restatement of the contract, upload of the per-observation arrays (keypoints and counts are taken to be
on the host already; median of --host-repeats runs).  The host route's arrays are compared with the device's.  Prints one JSON
object per configuration; --out FILE also writes them as text.

  python tools/track_extend_probe.py --out profiles/track_extend.txt"""
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

PARTS = ("ext_state", "ext_sort_points", "ext_runs", "link_init", "link_union", "link_label", "ext_sort_labels", "link_runs", "ext_flags",
         "ext_scan", "ext_emit")
NEW_LINKS, MIN_VIEWS = 400, 2
SHORT, CONFLICT, NO_ROW, REJECTED = -1, -2, -3, -4


def add_new_pairs(s, seed=2):
    """The pairs (q, q + 1) among the new frames (see the module text), appended to the pair arrays of the scene."""
    rng = np.random.default_rng(seed)
    first_new = N_FRAMES - N_NEW
    answered = np.zeros((N_FRAMES, CAP), bool)
    for p, q in enumerate(s["pair_q"]):
        answered[q] |= s["idx1"][p] >= 0
    idx1 = np.full((N_NEW - 1, CAP), -1, np.int32)
    for k in range(N_NEW - 1):
        q = first_new + k
        a = rng.permutation(np.flatnonzero(~answered[q]))[:NEW_LINKS]
        b = rng.permutation(np.flatnonzero(~answered[q + 1]))[:NEW_LINKS]
        n = min(len(a), len(b))
        idx1[k, a[:n]] = b[:n]
    pq = np.arange(first_new, N_FRAMES - 1, dtype=np.int32)
    return dict(s, pair_q=np.concatenate([s["pair_q"], pq]), pair_t=np.concatenate([s["pair_t"], pq + 1]),
                idx1=np.concatenate([s["idx1"], idx1]), keep=np.concatenate([s["keep"], np.ones_like(idx1, np.uint8)]))


def host_extend(s, idx1, inlier, node_point, row_point, row_inlier, n_points):
    """The numpy / scipy restatement a user had to write -> dict of arrays cut to their counts."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F, cap = N_FRAMES, CAP
    N = F * cap
    cnt = np.clip(s["counts"].astype(np.int64), 0, cap)
    nodes = np.arange(N)
    frame = nodes // cap
    exists = (nodes - frame * cap) < cnt[frame]
    mapped = exists & (node_point >= 0) & (node_point < n_points)
    claim = exists & ~mapped & (row_inlier != 0) & (row_point >= 0) & (row_point < n_points)
    out = np.full(N, NO_ROW, np.int64)
    out[mapped] = node_point[mapped]
    held = np.flatnonzero(mapped | claim)
    point = np.where(mapped[held], node_point[held], row_point[held]).astype(np.int64)
    _, inverse, count = np.unique(frame[held] * (n_points + 1) + point, return_inverse=True, return_counts=True)
    crowded = count[inverse] > 1
    is_claim = claim[held]
    out[held[is_claim & crowded]] = REJECTED
    out[held[is_claim & ~crowded]] = point[is_claim & ~crowded]
    n_adopted, n_rejected = int((is_claim & ~crowded).sum()), int((is_claim & crowded).sum())
    free = exists & ~mapped & ~claim

    q, t = s["pair_q"].astype(np.int64), s["pair_t"].astype(np.int64)
    i = np.arange(cap)[None, :]
    j = idx1.astype(np.int64)
    ok = ((q != t) & (q >= 0) & (q < F) & (t >= 0) & (t < F))[:, None] & (i < cnt[q][:, None]) & (inlier != 0) & (j >= 0) & (j < cnt[t][:, None])
    p, r = np.nonzero(ok)
    u, v = q[p] * cap + r, t[p] * cap + j[p, r]
    both = free[u] & free[v]
    u, v = u[both], v[both]
    _, lab = connected_components(coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(N, N)), directed=False)
    fn = np.flatnonzero(free)                                  # ascending: the first node of a component is its label
    comp, first, inv, size = np.unique(lab[fn], return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((frame[fn], inv))
    twice = (inv[order][1:] == inv[order][:-1]) & (frame[fn][order][1:] == frame[fn][order][:-1])
    conflict = np.zeros(len(comp), bool)
    conflict[inv[order][1:][twice]] = True
    track = ~conflict & (size >= MIN_VIEWS)
    by_label = np.argsort(first, kind="stable")
    new_id = np.full(len(comp), -1, np.int64)
    new_id[by_label[track[by_label]]] = n_points + np.arange(int(track.sum()))
    code = np.where(conflict, CONFLICT, np.where(track, new_id, SHORT))
    out[fn] = code[inv]
    obs_node = np.flatnonzero(out >= 0)
    fx, fy, cx, cy = INTRINSICS
    pix = s["kps"].reshape(-1, 7)[obs_node, :2].astype(np.float64)
    n_total = n_points + int(track.sum())
    return dict(node_point=out.astype(np.int32), obs_cam=(obs_node // cap).astype(np.int32), obs_point=out[obs_node].astype(np.int32),
                obs_xy=np.stack([(pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy], axis=1), obs_node=obs_node.astype(np.int32),
                point_len=np.bincount(out[obs_node], minlength=n_total).astype(np.int32),
                totals=[len(obs_node), n_total, n_adopted, n_rejected, int(conflict.sum()), int((~conflict & ~track & (size >= 2)).sum())])


def measure(ctx, name, repeats, host_repeats):
    import torch
    s = add_new_pairs(synth_map(CONFIGS[name]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    n_points, P = len(s["point_xyz"]), len(s["pair_q"])
    n_loc = P - (N_NEW - 1)  # the localisation sees the new-versus-map pairs only
    loc = estimator.localize_pairs(ctx, d["kps"], d["counts"], d["pair_q"][:n_loc].contiguous(), d["pair_t"][:n_loc].contiguous(),
                                   d["idx1"][:n_loc].contiguous(), d["keep"][:n_loc].contiguous(), d["node_point"], d["point_xyz"],
                                   d["status"], INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    # (allocations and the scratch's growth outside the timed windows)
    out = estimator.extend_tracks(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["keep"], d["node_point"], n_points,
                                  loc["row_point"], loc["row_inlier"], INTRINSICS, MIN_VIEWS)
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    args = [ctx.h, pv(d["kps"]), pv(d["counts"]), N_FRAMES, CAP, pv(d["pair_q"]), pv(d["pair_t"]), P, pv(d["idx1"]), pv(d["keep"]),
            pv(d["node_point"]), n_points, pv(loc["row_point"]), pv(loc["row_inlier"])] + [C.c_double(v) for v in INTRINSICS] + [MIN_VIEWS]

    def extend():
        ctx.check(hip.lib.gh_extend_tracks_dev(*args, *(pv(out[k]) for k in out)))
        torch.cuda.synchronize()

    extend_us = median(extend, repeats, 5)
    ctx.prof_enable(True)
    for _ in range(repeats):
        extend()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}

    t_host, t_down, h = [], [], None
    for rep in range(host_repeats + 1):
        t0 = time.perf_counter()
        idx1, keep, node_point = d["idx1"].cpu().numpy(), d["keep"].cpu().numpy(), d["node_point"].cpu().numpy()
        row_point, row_inlier = loc["row_point"].cpu().numpy(), loc["row_inlier"].cpu().numpy()
        t1 = time.perf_counter()
        h = host_extend(s, idx1, keep, node_point, row_point, row_inlier, n_points)
        up = [dev(h[k]) for k in ("node_point", "obs_cam", "obs_point", "obs_xy", "obs_node", "point_len")]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:  # (the first run warms the allocator)
            t_down.append(t1 - t0)
            t_host.append(t2 - t0)
        del up
    totals = out["totals"].cpu().numpy().tolist()
    n_obs, n_total = totals[:2]
    same = bool(h["totals"] == totals and np.array_equal(h["node_point"], out["node_point"].cpu().numpy()) and
                all(h[k].tobytes() == out[k][:n_obs].cpu().numpy().tobytes() for k in ("obs_cam", "obs_point", "obs_xy", "obs_node")) and
                np.array_equal(h["point_len"], out["point_len"][:n_total].cpu().numpy()) and not out["point_len"][n_total:].any().item() and
                int(out["point_new"].sum().item()) == n_total - n_points)
    return {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "new_frames": N_NEW, "pairs": P,
            "nodes": N_FRAMES * CAP, "rows": P * CAP, "map_points": n_points,
            "totals_obs_points_adopted_rejected_conflict_short": totals, "new_points": n_total - n_points,
            "grown_points": int(out["point_grew"].sum().item()), "extend_us": extend_us, "extend_parts_us": parts,
            "parts_sum_us": round(sum(parts.values()), 1), "host_download_us": stats(t_down), "host_route_us": stats(t_host),
            "host_route_over_extend": round(float(np.median(t_host)) * 1e6 / extend_us["median"], 1),
            "host_route_gives_the_same_arrays": same}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="map1,map2,map3")
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
            f.write("tools/track_extend_probe.py: the map extended by newly registered frames, gh_extend_tracks_dev "
                    "(synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
