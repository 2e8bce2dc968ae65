"""Track building from pair matches (gh_link_tracks_dev) on a sequence and on an all-pairs set.  Perf probe, not part of the
product.

  seq1 / seq2 / seq3   1000 frames x cap 2000, every frame paired with its next 1 / 2 / 3 neighbours
  all50                50 frames x cap 2000, all 1225 pairs

The matches are SYNTHETIC: ground-truth points, each visible over a window of 2 .. 20 consecutive frames (2 .. 50 for all50) at
a random row of every frame it is seen in, enough of them to fill about 90 % of the rows; idx1 of a pair links the two rows of
every point both frames see; 3 % of the matched rows are redirected to a random row of the train frame (wrong matches, the
source of CONFLICT components) and 2 % of the inlier bytes are 0.

Per configuration: the median of the whole call (device-resident, ended by a synchronise) over 20 calls after a warm-up; from
gh_prof_* in a run of its own (event timing slows the host side) the parts; and, on the same machine, the route a user had
before this entry: download idx1 and the mask, scipy.sparse.csgraph.connected_components plus the numpy grouping, upload
obs_cam / obs_point / obs_xy (the keypoints are taken to be on the host already; median of --host-repeats runs).  The host
route's result is compared with the device's.  Prints one JSON object per configuration; --out FILE also writes them as text.

  python tools/track_link_probe.py --out profiles/track_link.txt"""
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
CONFIGS = {"seq1": (1000, 2000, 1, 20), "seq2": (1000, 2000, 2, 20), "seq3": (1000, 2000, 3, 20), "all50": (50, 2000, 49, 50)}
PARTS = ("link_init", "link_union", "link_label", "link_sort", "link_runs", "link_flags", "link_scan", "link_emit")


def synth_matches(n_frames, cap, reach, max_window, seed=1, fill=0.9, wrong=0.03, masked=0.02):
    """-> kps (F x cap x 7 float32), counts, pair_q, pair_t, idx1 (P x cap), inlier (P x cap): see the module text."""
    rng = np.random.default_rng(seed)
    max_window = min(max_window, n_frames)
    n_points = int(n_frames * cap * fill / ((2 + max_window) / 2))
    length = rng.integers(2, max_window + 1, n_points)
    first = (rng.random(n_points) * (n_frames - length + 1)).astype(np.int64)
    o_point = np.repeat(np.arange(n_points), length)
    o_frame = np.repeat(first, length) + (np.arange(len(o_point)) - np.repeat(np.cumsum(length) - length, length))
    order = np.lexsort((rng.random(len(o_point)), o_frame))  # by frame, random inside a frame
    o_point, o_frame = o_point[order], o_frame[order]
    per_frame = np.bincount(o_frame, minlength=n_frames)
    o_row = np.arange(len(o_point)) - np.repeat(np.cumsum(per_frame) - per_frame, per_frame)
    keep = o_row < cap
    o_point, o_frame, o_row = o_point[keep], o_frame[keep], o_row[keep]
    counts = np.minimum(per_frame, cap).astype(np.int32)
    key = o_point * n_frames + o_frame
    by_key = np.argsort(key)
    key_sorted = key[by_key]
    pairs = [(f, f + d) for d in range(1, reach + 1) for f in range(n_frames - d)]
    pair_base = np.cumsum([0] + [n_frames - d for d in range(1, reach + 1)])
    idx1 = np.full((len(pairs), cap), -1, np.int32)
    for d in range(1, reach + 1):
        want = key + d  # the same point in frame + d
        pos = np.minimum(np.searchsorted(key_sorted, want), len(key_sorted) - 1)
        hit = (key_sorted[pos] == want) & (o_frame + d < n_frames)
        idx1[pair_base[d - 1] + o_frame[hit], o_row[hit]] = o_row[by_key[pos[hit]]]
    pq = np.array([p[0] for p in pairs], np.int32)
    pt = np.array([p[1] for p in pairs], np.int32)
    redirect = (idx1 >= 0) & (rng.random(idx1.shape) < wrong)
    rnd = (rng.random(idx1.shape) * np.maximum(counts[pt], 1)[:, None]).astype(np.int32)
    idx1[redirect] = rnd[redirect]
    inlier = (rng.random(idx1.shape) >= masked).astype(np.uint8)
    kps = np.zeros((n_frames, cap, 7), np.float32)
    kps[..., 0] = rng.uniform(0, 640, (n_frames, cap))
    kps[..., 1] = rng.uniform(0, 480, (n_frames, cap))
    return kps, counts, pq, pt, idx1, inlier


def host_route(kps_xy, counts, pq, pt, idx1_dev, inlier_dev, cap, min_views=2):
    """What a user had to do before gh_link_tracks_dev -> (obs_cam, obs_point, obs_xy on the device, n_points)."""
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    idx1, inl = idx1_dev.cpu().numpy(), inlier_dev.cpu().numpy()
    n_frames = len(counts)
    N = n_frames * cap
    cnt = np.clip(counts, 0, cap)
    rows = np.arange(cap)[None, :]
    ok = (rows < cnt[pq][:, None]) & (inl != 0) & (idx1 >= 0) & (idx1 < cnt[pt][:, None])
    p, i = np.nonzero(ok)
    u, v = pq[p].astype(np.int64) * cap + i, pt[p].astype(np.int64) * cap + idx1[p, i]
    _, lab = connected_components(coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(N, N)), directed=False)
    nodes = np.flatnonzero((np.arange(N) % cap) < cnt[np.arange(N) // cap])
    order = np.argsort(lab[nodes], kind="stable")
    sn, sl = nodes[order], lab[nodes][order]            # grouped by component, ascending node id inside one
    head = np.r_[True, sl[1:] != sl[:-1]]
    comp = np.cumsum(head) - 1
    size = np.bincount(comp)
    clash = np.r_[(sl[1:] == sl[:-1]) & (sn[1:] // cap == sn[:-1] // cap), False]
    bad = np.bincount(comp, weights=clash) > 0
    track = ~bad & (size >= min_views)
    first_node = sn[head]                               # the label: the smallest node id
    pid = np.full(len(size), -1, np.int64)
    t = np.flatnonzero(track)
    pid[t[np.argsort(first_node[t])]] = np.arange(len(t))
    node_pid = pid[comp]
    sel = np.flatnonzero(node_pid >= 0)
    sel = sel[np.argsort(sn[sel])]                      # observations in ascending node id
    on = sn[sel]
    fx, fy, cx, cy = INTRINSICS
    xy = kps_xy.reshape(-1, 2)[on].astype(np.float64)
    obs_xy = np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy], axis=1)
    out = (torch.from_numpy((on // cap).astype(np.int32)).cuda(), torch.from_numpy(node_pid[sel].astype(np.int32)).cuda(),
           torch.from_numpy(obs_xy).cuda())
    torch.cuda.synchronize()
    return out + (len(t),)


def median(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"median": round(float(np.median(t)) * 1e6, 1), "min": round(min(t) * 1e6, 1), "max": round(max(t) * 1e6, 1), "repeats": n}


def measure(ctx, name, repeats, host_repeats):
    import torch
    n_frames, cap, reach, window = CONFIGS[name]
    kps, counts, pq, pt, idx1, inlier = synth_matches(n_frames, cap, reach, window)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [dev(a) for a in (kps, counts, pq, pt, idx1, inlier)]
    out = estimator.link_tracks(ctx, *d, INTRINSICS)  # (allocations and the scratch's growth outside the timed window)
    pv = lambda x: C.c_void_p(x.data_ptr())
    fx, fy, cx, cy = INTRINSICS

    def call():
        ctx.check(hip.lib.gh_link_tracks_dev(ctx.h, pv(d[0]), pv(d[1]), n_frames, cap, pv(d[2]), pv(d[3]), len(pq), pv(d[4]), pv(d[5]),
                                             C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), 2,
                                             *(pv(out[k]) for k in out)))
        torch.cuda.synchronize()

    call_us = median(call, repeats, 5)
    ctx.prof_enable(True)
    for _ in range(repeats):
        call()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}
    host = {}
    host_us = median(lambda: host.update(r=host_route(kps[..., :2], counts, pq, pt, d[4], d[5], cap)), host_repeats, 1)
    totals = out["totals"].cpu().numpy().tolist()
    n_obs, n_points = totals[:2]
    h_cam, h_point, h_xy, h_points = host["r"]
    same = bool(h_points == n_points and len(h_cam) == n_obs and torch.equal(h_cam, out["obs_cam"][:n_obs]) and
                torch.equal(h_point, out["obs_point"][:n_obs]) and torch.equal(h_xy, out["obs_xy"][:n_obs]))
    plen = out["point_len"].cpu().numpy()[:n_points]
    return {"config": name, "device": ctx.device_info()["name"], "frames": n_frames, "cap": cap, "pairs": len(pq), "nodes": n_frames * cap,
            "rows": int(len(pq)) * cap, "edges": int(((idx1 >= 0) & (inlier != 0)).sum()),
            "totals_obs_points_conflict_short": totals, "track_length_median_max": [float(np.median(plen)), int(plen.max())] if n_points else None,
            "call_us": call_us, "parts_us": parts, "host_route_us": host_us, "host_route_over_device": round(host_us["median"] / call_us["median"], 1),
            "host_route_gives_the_same_arrays": same}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="seq1,seq2,seq3,all50")
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
            f.write("tools/track_link_probe.py: tracks from pair matches, gh_link_tracks_dev (synthetic matches; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
