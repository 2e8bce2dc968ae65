"""Registering new frames against the map (gh_pnp_gather_pairs_dev, gh_localize_pairs_dev).  Perf probe, not part of the product.

  map1 / map2 / map3   1000 frames x cap 2000; each of the last 100 frames matched against 1 / 2 / 3 map frames

The scene is SYNTHETIC but geometrically consistent, so that the PnP stage does real work: every new frame looks down +z from
a random position near the origin at 1500 points of its own, 4 .. 8 units away, its keypoints are their projections plus half a
pixel of noise at random rows; each of its map frames holds a random 70 % of those points at random rows of node_point; idx1 of
a pair links the two rows of every point both frames hold; 3 % of the matched rows are redirected to a random row of the map
frame, 2 % of the keep bytes are 0, 5 % of the points are not GH_TRACK_OK, and node_point is dirty where no point sits.

Per configuration: the median of the whole gather and of the composed call (device-resident, ended by a synchronise) over 20
calls after a warm-up, with the range; from gh_prof_* in a run of its own (event timing slows the host side) the parts of the
gather; and, on the same machine in the same run, the route a user had before these entries: download idx1, keep and
node_point, the numpy gather, upload xyz / xy / offsets, then pnp_batch (keypoints, points and status are taken to be on the
host already; median of --host-repeats runs).  The host route's arrays are compared with the device's.  Prints one JSON object
per configuration; --out FILE also writes them as text.

  python tools/localize_probe.py --out profiles/localize.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gslam_amd import estimator, hip  # noqa: E402

INTRINSICS = (517.3, 516.5, 318.6, 255.3)
CONFIGS = {"map1": 1, "map2": 2, "map3": 3}
N_FRAMES, CAP, N_NEW, PER_FRAME = 1000, 2000, 100, 1500
PARTS = ("loc_init", "loc_vote", "loc_key", "loc_sort", "loc_runs", "loc_flags", "loc_scan", "loc_emit")
RANSAC_THRESHOLD, INLIER_THRESHOLD, SEED = 0.006, 0.006, 7


def synth_map(reach, seed=1, held=0.7, wrong=0.03, masked=0.02, not_ok=0.05, noise_px=0.5):
    """-> dict of host arrays: kps, counts, pair_q, pair_t, idx1, keep, node_point, point_xyz, status, positions (see the module
    text)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = INTRINSICS
    n_points = N_NEW * PER_FRAME
    kps = np.zeros((N_FRAMES, CAP, 7), np.float32)
    kps[..., 0] = rng.uniform(0, 640, (N_FRAMES, CAP))
    kps[..., 1] = rng.uniform(0, 480, (N_FRAMES, CAP))
    counts = np.full(N_FRAMES, CAP, np.int32)
    dirt = np.array([-1, -2, -3, n_points, 2**31 - 1], np.int64)
    node_point = dirt[rng.integers(0, len(dirt), (N_FRAMES, CAP))]
    point_xyz = np.zeros((n_points, 3))
    positions = rng.uniform(-0.3, 0.3, (N_FRAMES, 3))
    pairs, rows_q, rows_t = [], [], []
    first_new = N_FRAMES - N_NEW
    for k in range(N_NEW):
        q = first_new + k
        ids = np.arange(k * PER_FRAME, (k + 1) * PER_FRAME)
        Xc = np.stack([rng.uniform(-2, 2, PER_FRAME), rng.uniform(-1.5, 1.5, PER_FRAME), rng.uniform(4, 8, PER_FRAME)], axis=1)
        point_xyz[ids] = Xc + positions[q]
        row_q = rng.permutation(CAP)[:PER_FRAME]
        kps[q, row_q, 0] = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(0, noise_px, PER_FRAME)
        kps[q, row_q, 1] = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(0, noise_px, PER_FRAME)
        for d in range(1, reach + 1):
            t = q - N_NEW * d
            has = np.flatnonzero(rng.random(PER_FRAME) < held)
            row_t = rng.permutation(CAP)[:len(has)]
            node_point[t, row_t] = ids[has]
            pairs.append((q, t))
            rows_q.append(row_q[has])
            rows_t.append(row_t)
    idx1 = np.full((len(pairs), CAP), -1, np.int32)
    for p in range(len(pairs)):
        idx1[p, rows_q[p]] = rows_t[p]
    redirect = (idx1 >= 0) & (rng.random(idx1.shape) < wrong)
    idx1[redirect] = rng.integers(0, CAP, idx1.shape)[redirect]
    keep = (rng.random(idx1.shape) >= masked).astype(np.uint8)
    status = np.where(rng.random(n_points) < not_ok, 3, 0).astype(np.int32)
    return dict(kps=kps, counts=counts, pair_q=np.array([p[0] for p in pairs], np.int32), pair_t=np.array([p[1] for p in pairs], np.int32),
                idx1=idx1, keep=keep, node_point=node_point.astype(np.int32).reshape(-1), point_xyz=point_xyz, status=status,
                positions=positions)


def host_gather(s, idx1, keep, node_point):
    """The numpy gather a user had to write -> (xyz n_corr x 3, xy n_corr x 2, offsets F + 1, corr_node n_corr)."""
    F, cap = N_FRAMES, CAP
    N, n_points = F * cap, len(s["point_xyz"])
    cnt = np.clip(s["counts"].astype(np.int64), 0, cap)
    q, t = s["pair_q"].astype(np.int64), s["pair_t"].astype(np.int64)
    i = np.arange(cap)[None, :]
    j = idx1.astype(np.int64)
    ok = ((q != t) & (q >= 0) & (q < F) & (t >= 0) & (t < F))[:, None] & (i < cnt[q][:, None]) & (keep != 0) & (j >= 0) & (j < cnt[t][:, None])
    p, r = np.nonzero(ok)
    cand = node_point.astype(np.int64)[t[p] * cap + j[p, r]]
    node = q[p] * cap + r
    good = (cand >= 0) & (cand < n_points)
    node, cand = node[good], cand[good]
    good = s["status"][cand] == 0
    node, cand = node[good], cand[good]
    order = np.lexsort((cand, node))                      # by node, ascending candidate inside one
    node, cand = node[order], cand[order]
    head = np.r_[True, node[1:] != node[:-1]]
    tail = np.r_[node[1:] != node[:-1], True]
    claim_node, lo, hi = node[head], cand[head], cand[tail]
    one = lo == hi
    claim_node, claim = claim_node[one], lo[one]
    key = (claim_node // cap) * (n_points + 1) + claim    # (frame, point)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    dup = np.r_[False, ks[1:] == ks[:-1]] | np.r_[ks[1:] == ks[:-1], False]
    alone = np.ones(len(key), bool)
    alone[order[dup]] = False
    corr_node, point = claim_node[alone], claim[alone]     # (ascending node id already)
    fx, fy, cx, cy = INTRINSICS
    pix = s["kps"].reshape(-1, 7)[corr_node, :2].astype(np.float64)
    xy = np.stack([(pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy], axis=1)
    offsets = np.r_[0, np.cumsum(np.bincount(corr_node // cap, minlength=F))].astype(np.int32)
    return np.ascontiguousarray(s["point_xyz"][point]), np.ascontiguousarray(xy), offsets, corr_node.astype(np.int32)


def stats(t):
    return {"median": round(float(np.median(t)) * 1e6, 1), "min": round(min(t) * 1e6, 1), "max": round(max(t) * 1e6, 1), "repeats": len(t)}


def median(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return stats(t)


def measure(ctx, name, repeats, host_repeats):
    import torch
    s = synth_map(CONFIGS[name])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    args = [d[k] for k in ("kps", "counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")]
    # (allocations and the scratch's growth outside the timed windows)
    loc = estimator.localize_pairs(ctx, *args, INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    out = estimator.gather_map_matches(ctx, *args, INTRINSICS)
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    n_points = len(s["point_xyz"])
    head = [ctx.h, pv(d["kps"]), pv(d["counts"]), N_FRAMES, CAP, pv(d["pair_q"]), pv(d["pair_t"]), len(s["pair_q"]), pv(d["idx1"]),
            pv(d["keep"]), pv(d["node_point"]), n_points, pv(d["point_xyz"]), pv(d["status"])] + [C.c_double(v) for v in INTRINSICS]
    opt = hip.BaOptions()
    hip.lib.gh_ba_default_options(C.byref(opt))

    def gather():
        ctx.check(hip.lib.gh_pnp_gather_pairs_dev(*head, *(pv(out[k]) for k in out)))
        torch.cuda.synchronize()

    def composed():
        ctx.check(hip.lib.gh_localize_pairs_dev(*head, C.c_double(RANSAC_THRESHOLD), C.c_uint64(SEED), 63, C.byref(opt), 0,
                                                C.c_double(INLIER_THRESHOLD), *(pv(loc[k]) for k in loc)))
        torch.cuda.synchronize()

    def pnp_only():
        estimator.pnp_batch(ctx, out["xyz"], out["xy"], out["offsets"], RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
        torch.cuda.synchronize()

    gather_us = median(gather, repeats, 5)
    composed_us = median(composed, repeats, 5)
    pnp_us = median(pnp_only, repeats, 3)
    ctx.prof_enable(True)
    for _ in range(repeats):
        gather()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}

    host, t_gather, t_all = {}, [], []
    for rep in range(host_repeats + 1):
        t0 = time.perf_counter()
        idx1, keep, node_point = d["idx1"].cpu().numpy(), d["keep"].cpu().numpy(), d["node_point"].cpu().numpy()
        xyz, xy, offsets, corr_node = host_gather(s, idx1, keep, node_point)
        h = [dev(xyz), dev(xy), dev(offsets)]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host["pnp"] = estimator.pnp_batch(ctx, *h, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:  # (the first run warms the allocator)
            t_gather.append(t1 - t0)
            t_all.append(t2 - t0)
        host["r"] = (xyz, xy, offsets, corr_node)
    totals = out["totals"].cpu().numpy().tolist()
    n_corr = totals[0]
    xyz, xy, offsets, corr_node = host["r"]
    same = bool(len(xyz) == n_corr and np.array_equal(offsets, out["offsets"].cpu().numpy()) and
                xyz.tobytes() == out["xyz"][:n_corr].cpu().numpy().tobytes() and xy.tobytes() == out["xy"][:n_corr].cpu().numpy().tobytes() and
                np.array_equal(corr_node, out["corr_node"][:n_corr].cpu().numpy()))
    same_poses = bool(torch.equal(host["pnp"]["poses"], loc["poses"]))
    new = slice(N_FRAMES - N_NEW, N_FRAMES)
    poses = loc["poses"].cpu().numpy()[new]
    row_inlier = loc["row_inlier"].cpu().numpy()
    return {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "new_frames": N_NEW, "pairs": len(s["pair_q"]),
            "nodes": N_FRAMES * CAP, "rows": int(len(s["pair_q"])) * CAP, "map_points": n_points,
            "totals_corr_ambiguous_shared_frames": totals, "inlier_rows": int(row_inlier.sum()),
            "position_error_median_max": [float(np.median(np.linalg.norm(poses[:, 4:] - s["positions"][new], axis=1))),
                                          float(np.linalg.norm(poses[:, 4:] - s["positions"][new], axis=1).max())],
            "gather_us": gather_us, "gather_parts_us": parts, "localize_us": composed_us, "pnp_batch_alone_us": pnp_us,
            "host_gather_us": stats(t_gather), "host_route_us": stats(t_all),
            "host_gather_over_device_gather": round(float(np.median(t_gather)) * 1e6 / gather_us["median"], 1),
            "host_route_over_localize": round(float(np.median(t_all)) * 1e6 / composed_us["median"], 1),
            "host_gather_gives_the_same_arrays": same, "host_route_gives_the_same_poses": same_poses}


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
            f.write("tools/localize_probe.py: new frames against the map, gh_pnp_gather_pairs_dev / gh_localize_pairs_dev "
                    "(synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
