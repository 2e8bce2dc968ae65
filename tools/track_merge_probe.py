"""Merging map points that the matches show to be one (gh_merge_points_dev).  Perf probe, not part of the product.

  map1   1000 frames x cap 2000, the last 100 new, each matched against 1 map frame (row 1 of tools/track_extend_probe.py)

The scene is the one of tools/track_extend_probe.py after a real gh_localize_pairs_dev -> gh_extend_tracks_dev (outside the
timed windows).  Before the call 5 % of the map points with at least 4 observations are split into two ids on the host: the
later half of a point's nodes gets an id above all others and the coordinates are copied.  The call gets the pair arrays of
the extension; the gate is on (max_dist 0.1; a split copy is at distance 0), every point counts as usable.

Reported: the median of the whole call (device-resident, ended by a synchronise) over 20 calls after a warm-up, with the range;
from gh_prof_* in a run of its own (event timing slows the host side) the parts; and, on the same machine in the same run, the
route a user had before this entry: download node_point, idx1 and the inlier bytes, a vectorised numpy / scipy restatement of
the contract, upload of the remap table, node_point, obs_point and point_len (counts, the coordinates and obs_point are taken to
be on the host already; median of --host-repeats runs).  The host route's arrays are compared with the device's.  Prints one
JSON object; --out FILE also writes it as text.

  python tools/track_merge_probe.py --out profiles/track_merge.txt"""
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

PARTS = ("mrg_init", "mrg_union", "mrg_label", "mrg_key", "mrg_sort", "mrg_runs", "mrg_points", "mrg_emit")
SPLIT_SHARE, MIN_OBS, MAX_DIST = 0.05, 4, 0.1
OUTPUTS = ("point_remap", "point_state", "point_select", "node_point", "obs_point", "point_len", "totals")


def split_points(node_point, exists, n_used, xyz, seed=3):
    """5 % of the points with at least MIN_OBS existing nodes: the later half of their nodes gets the ids n_used, n_used + 1, ...
    and the coordinates of the point they came from.  -> (node_point, xyz, number of splits)."""
    rng = np.random.default_rng(seed)
    held = np.flatnonzero(exists & (node_point >= 0) & (node_point < n_used))
    order = held[np.argsort(node_point[held], kind="stable")]           # by point, ascending node inside a point
    ids, start, count = np.unique(node_point[order], return_index=True, return_counts=True)
    long = np.flatnonzero(count >= MIN_OBS)
    chosen = np.sort(rng.permutation(long)[:int(len(long) * SPLIT_SHARE)])
    out, xyz = node_point.copy(), xyz.copy()
    for k, c in enumerate(chosen):
        out[order[start[c] + count[c] // 2:start[c] + count[c]]] = n_used + k
        xyz[n_used + k] = xyz[ids[c]]
    return out, xyz, len(chosen)


def host_merge(s, idx1, inlier, node_point, n_points, xyz, obs_point):
    """The numpy / scipy restatement a user had to write (every point usable, BRIDGE nodes on) -> dict of arrays."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F, cap = N_FRAMES, CAP
    N = F * cap
    cnt = np.clip(s["counts"].astype(np.int64), 0, cap)
    nodes = np.arange(N)
    frame = nodes // cap
    exists = (nodes - frame * cap) < cnt[frame]
    v = node_point.astype(np.int64)
    holder = exists & (v >= 0) & (v < n_points)
    elem = np.where(holder, v, np.where(exists, n_points + nodes, -1))
    q, t = s["pair_q"].astype(np.int64), s["pair_t"].astype(np.int64)
    i = np.arange(cap)[None, :]
    j = idx1.astype(np.int64)
    ok = ((q != t) & (q >= 0) & (q < F) & (t >= 0) & (t < F))[:, None] & (i < cnt[q][:, None]) & (inlier != 0) & (j >= 0) & (j < cnt[t][:, None])
    p, r = np.nonzero(ok)
    a, b = elem[q[p] * cap + r], elem[t[p] * cap + j[p, r]]
    keep = (a >= 0) & (b >= 0) & (a != b)
    a, b = a[keep], b[keep]
    E = n_points + N
    _, lab = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(E, E)), directed=False)
    plab = lab[:n_points]
    first = np.full(lab.max() + 1, n_points, np.int64)
    np.minimum.at(first, plab, np.arange(n_points))                      # the smallest point of every component
    size = np.bincount(plab, minlength=len(first))
    label = first[plab]
    grouped = size[plab] >= 2
    h = np.flatnonzero(holder & grouped[np.clip(v, 0, n_points - 1)])
    key = label[v[h]] * F + frame[h]
    key.sort()
    conflict = np.zeros(n_points, bool)
    conflict[key[1:][key[1:] == key[:-1]] // F] = True
    d = xyz - xyz[label]
    near = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= MAX_DIST * MAX_DIST
    far = np.zeros(n_points, bool)
    far[label[grouped & ~near]] = True
    merged = grouped & ~conflict[label] & ~far[label]
    remap = np.where(merged, label, np.arange(n_points))
    state = np.where(~grouped, 0, np.where(conflict[label], 3, np.where(far[label], 4, np.where(label == np.arange(n_points), 1, 2))))
    rename = lambda x: np.where((x >= 0) & (x < n_points), remap[np.clip(x, 0, n_points - 1)], x)
    out = rename(v)
    lead = (label == np.arange(n_points)) & grouped
    totals = [int((state == 1).sum()), int((state == 2).sum()), int((lead & (state == 3)).sum()), int((lead & (state == 4)).sum()),
              int((exists & (out != v)).sum()), int(((state == 3) | (state == 4)).sum())]
    return dict(point_remap=remap.astype(np.int32), point_state=state.astype(np.uint8), point_select=(state == 1).astype(np.uint8),
                node_point=out.astype(np.int32), obs_point=rename(obs_point.astype(np.int64)).astype(np.int32),
                point_len=np.bincount(out[holder], minlength=n_points).astype(np.int32), totals=np.array(totals, np.int32))


def measure(ctx, name, repeats, host_repeats):
    import torch
    s = add_new_pairs(synth_map(CONFIGS[name]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    n_map, P = len(s["point_xyz"]), len(s["pair_q"])
    n_loc = P - (N_NEW - 1)  # the localisation sees the new-versus-map pairs only
    loc = estimator.localize_pairs(ctx, d["kps"], d["counts"], d["pair_q"][:n_loc].contiguous(), d["pair_t"][:n_loc].contiguous(),
                                   d["idx1"][:n_loc].contiguous(), d["keep"][:n_loc].contiguous(), d["node_point"], d["point_xyz"],
                                   d["status"], INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    ext = estimator.extend_tracks(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["keep"], d["node_point"], n_map,
                                  loc["row_point"], loc["row_inlier"], INTRINSICS, MIN_VIEWS)
    N = N_FRAMES * CAP
    PC = n_map + N // 2
    n_used = int(ext["totals"].cpu().numpy()[1])
    cnt = np.clip(s["counts"].astype(np.int64), 0, CAP)
    exists = (np.arange(N) % CAP) < cnt[np.arange(N) // CAP]
    xyz = np.zeros((PC, 3))
    xyz[:n_map] = s["point_xyz"]
    node_point, xyz, n_split = split_points(ext["node_point"].cpu().numpy(), exists, n_used, xyz)
    held = np.flatnonzero(exists & (node_point >= 0) & (node_point < PC))
    obs_point = np.full(N, -1, np.int32)
    obs_point[:len(held)] = node_point[held]
    m_in = dict(node_point=dev(node_point), xyz=dev(xyz), obs_point=dev(obs_point))
    # (allocations and the scratch's growth outside the timed windows)
    out = estimator.merge_points(ctx, d["counts"], CAP, d["pair_q"], d["pair_t"], d["idx1"], d["keep"], m_in["node_point"], PC,
                                 point_xyz=m_in["xyz"], max_dist=MAX_DIST, obs_point=m_in["obs_point"])
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    args = [ctx.h, pv(d["counts"]), N_FRAMES, CAP, pv(d["pair_q"]), pv(d["pair_t"]), P, pv(d["idx1"]), pv(d["keep"]), pv(m_in["node_point"]), PC,
            None, pv(m_in["xyz"]), C.c_double(MAX_DIST), 1, pv(m_in["obs_point"])]

    def merge():
        ctx.check(hip.lib.gh_merge_points_dev(*args, *(pv(out[k]) for k in OUTPUTS)))
        torch.cuda.synchronize()

    merge_us = median(merge, repeats, 5)
    ctx.prof_enable(True)
    for _ in range(repeats):
        merge()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}

    t_host, t_down, h = [], [], None
    for rep in range(host_repeats + 1):
        t0 = time.perf_counter()
        idx1, keep, np_host = d["idx1"].cpu().numpy(), d["keep"].cpu().numpy(), m_in["node_point"].cpu().numpy()
        t1 = time.perf_counter()
        h = host_merge(s, idx1, keep, np_host, PC, xyz, obs_point)
        up = [dev(h[k]) for k in ("point_remap", "node_point", "obs_point", "point_len")]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:  # (the first run warms the allocator)
            t_down.append(t1 - t0)
            t_host.append(t2 - t0)
        del up
    same = {k: bool(h[k].tobytes() == out[k].cpu().numpy().tobytes()) for k in OUTPUTS}
    return {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "new_frames": N_NEW, "pairs": P,
            "nodes": N, "rows": P * CAP, "point_capacity": PC, "points_in_use": n_used + n_split, "points_split": n_split,
            "totals_merged_absorbed_conflict_far_changed_apart": out["totals"].cpu().numpy().tolist(), "merge_us": merge_us,
            "merge_parts_us": parts, "parts_sum_us": round(sum(parts.values()), 1), "host_download_us": stats(t_down),
            "host_route_us": stats(t_host), "host_route_over_merge": round(float(np.median(t_host)) * 1e6 / merge_us["median"], 1),
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
            f.write("tools/track_merge_probe.py: map points that the matches show to be one, gh_merge_points_dev "
                    "(synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
