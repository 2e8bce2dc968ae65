"""Search by projection (gh_search_projection_dev).  Perf probe, not part of the product.

  map1   1000 frames x cap 2000, the last 100 new, each matched against 1 map frame (row 1 of tools/track_extend_probe.py)

The scene is the one of tools/localize_probe.py: the map before the new frames join it.  Its observation list is written out
from node_point (one observation per mapped node), gh_describe_points_dev gives the 150 000 points their summaries, a real
gh_localize_pairs_dev gives the new frames their poses and claims, and the search runs between that call and the extension, on
the last 10 and on all 100 new frames, into output arrays of its own so that every call sees the same inputs.  The descriptors
are synthetic (random bytes: the Hamming gate turns nearly every window down, as it does for a wrong match), the octaves random
in 0 .. 7.  Every camera looks down +z from within 0.3 of the origin, so nearly every point projects into every searched frame.

Reported: the median of the whole call (device-resident, ended by a synchronise) over 20 calls after a warm-up, with the range;
from gh_prof_* in a run of its own (event timing slows the host side) the parts of the call; and, on the same machine in the
same run, the route a user had before this entry, for the 10-frame call: download the keypoints, descriptors, poses, map, claims,
points and summaries, the contract in numpy with a 32-pixel grid over the open keypoints of a frame, upload of the three node
arrays (median of --host-repeats runs).  The host route's arrays are compared with the device's.  Prints one JSON object per
call size; --out FILE also writes them as text.

  python tools/search_projection_probe.py --out profiles/search_projection.txt"""
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

PARTS = ("sproj_frames", "sproj_grid", "sproj_index", "sproj_search", "sproj_resolve", "sproj_finish")
OUTPUTS = ("row_point", "row_inlier", "row_dist", "frame_totals", "totals")
SIZE = (640, 480)
CELL = 32
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)
LOC_NO_POINT, LOC_NO_ROW = -1, -3


def host_search(c, prm):
    """The contract in numpy with a grid, the route a user had to write.  c: dict of host arrays (kps F x cap x 7 float32, desc
    F x cap x 32, counts, poses, frame_search, node_point / row_point / row_inlier or None, n_points, xyz, status or None, select
    or None, views, point_desc, normal, dist, intrinsics, size); prm: dict of the parameters.  -> dict of the five outputs."""
    F, cap = c["kps"].shape[:2]
    N, P = F * cap, c["n_points"]
    fx, fy, cx, cy = c["intrinsics"]
    W, H = (float(v) for v in c["size"])
    gx, gy = -(-int(W) // CELL), -(-int(H) // CELL)
    x, y = c["kps"][..., 0].astype(np.float64), c["kps"][..., 1].astype(np.float64)
    octave = c["kps"][..., 5].copy().view(np.int32).astype(np.int64)
    exists = np.arange(cap)[None, :] < np.clip(c["counts"], 0, cap)[:, None]
    taken = np.full((F, cap), -1, np.int64)
    if c["row_point"] is not None:
        rp = c["row_point"].reshape(F, cap).astype(np.int64)
        m = exists & (c["row_inlier"].reshape(F, cap) != 0) & (rp >= 0) & (rp < P)
        taken[m] = rp[m]
    if c["node_point"] is not None:
        npt = c["node_point"].reshape(F, cap).astype(np.int64)
        m = exists & (npt >= 0) & (npt < P)
        taken[m] = npt[m]
    searchable = c["views"] > 0
    if c["select"] is not None:
        searchable = searchable & (c["select"] != 0)
    if c["status"] is not None:
        searchable = searchable & (c["status"] == 0)
    searched = np.flatnonzero(c["frame_search"] != 0)
    pw = np.ones(32)
    for l in range(1, 32):
        pw[l] = pw[l - 1] * prm["scale_factor"]
    ft = np.zeros((F, 10), np.int64)
    prop_node, prop_h, prop_p = [], [], []
    X, nrm = c["xyz"].reshape(P, 3), c["normal"].reshape(P, 3)
    min_dist, max_dist = c["dist"].reshape(P, 2)[:, 0], c["dist"].reshape(P, 2)[:, 1]
    pdesc, desc = c["point_desc"].reshape(P, 32), c["desc"].reshape(F, cap, 32)

    def cell(v, g):  # the clamp: monotone, NaN and negatives to 0
        with np.errstate(invalid="ignore"):
            return np.where(v >= 0, np.minimum(np.where(np.isfinite(v), v, 1e18) // CELL, g - 1), 0).astype(np.int64)

    with np.errstate(all="ignore"):
        for f in searched:
            q, t = c["poses"][f, :4], c["poses"][f, 4:]
            qc = np.array([-q[0], -q[1], -q[2], q[3]])
            d = X - t
            uvx, uvy, uvz = qc[1] * d[:, 2] - qc[2] * d[:, 1], qc[2] * d[:, 0] - qc[0] * d[:, 2], qc[0] * d[:, 1] - qc[1] * d[:, 0]
            uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
            Xc0 = d[:, 0] + qc[3] * uvx + (qc[1] * uvz - qc[2] * uvy)
            Xc1 = d[:, 1] + qc[3] * uvy + (qc[2] * uvx - qc[0] * uvz)
            Xc2 = d[:, 2] + qc[3] * uvz + (qc[0] * uvy - qc[1] * uvx)
            iz = 1.0 / Xc2
            u, v = fx * (Xc0 * iz) + cx, fy * (Xc1 * iz) + cy
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            cosv = ((d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]) / dist
            level = (pw[None, :max(prm["n_levels"] - 1, 0)] * dist[:, None] < max_dist[:, None]).sum(1)
            radius = (prm["radius_scale"] * np.where(cosv > prm["near_cos"], prm["radius_near"], prm["radius_far"])) * pw[level]
            held = np.zeros(P, bool)
            held[taken[f][taken[f] >= 0]] = True
            left = searchable.copy()
            for code, fails in ((0, held), (1, ~(Xc2 > 1e-9)), (2, ~((0.0 <= u) & (u < W) & (0.0 <= v) & (v < H))),
                                (3, ~((dist >= prm["range_lo"] * min_dist) & (dist <= prm["range_hi"] * max_dist))),
                                (4, ~(cosv >= prm["min_view_cos"]))):
                ft[f, code] = int((left & fails).sum())
                left &= ~fails
            surv = np.flatnonzero(left)
            # the grid: the open rows of the frame by cell, ascending row inside a cell
            rows = np.flatnonzero(exists[f] & (taken[f] < 0))
            key = cell(y[f][rows], gy) * gx + cell(x[f][rows], gx)
            order = np.argsort(key, kind="stable")
            rows, key = rows[order], key[order]
            start = np.searchsorted(key, np.arange(gx * gy + 1))
            us, vs, rs, ls = u[surv], v[surv], radius[surv], level[surv]
            cx_lo, cx_hi, cy_lo, cy_hi = cell(us - rs, gx), cell(us + rs, gx), cell(vs - rs, gy), cell(vs + rs, gy)
            who, which = [], []
            for k in range(int((cy_hi - cy_lo).max()) + 1 if len(surv) else 0):  # one grid row of every window at a time
                cyk = cy_lo + k
                on = cyk <= cy_hi
                b, e = start[(cyk * gx + cx_lo)[on]], start[(cyk * gx + cx_hi)[on] + 1]
                n = e - b
                owner = np.repeat(np.flatnonzero(on), n)
                offs = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
                who.append(owner)
                which.append(rows[np.repeat(b, n) + offs])
            who = np.concatenate(who) if who else np.zeros(0, np.int64)
            which = np.concatenate(which) if which else np.zeros(0, np.int64)
            ok = ((octave[f][which] >= ls[who] - 1) & (octave[f][which] <= ls[who]) & (np.abs(x[f][which] - us[who]) < rs[who]) &
                  (np.abs(y[f][which] - vs[who]) < rs[who]))
            who, which = who[ok], which[ok]
            h = POPCOUNT[desc[f][which] ^ pdesc[surv[who]]].sum(1)
            order = np.lexsort((which, h, who))
            who, which, h = who[order], which[order], h[order]
            first = np.flatnonzero(np.r_[True, who[1:] != who[:-1]]) if len(who) else np.zeros(0, np.int64)
            has_second = np.zeros(len(first), bool)
            if len(first):
                nxt = np.minimum(first + 1, len(who) - 1)
                has_second = (first + 1 < len(who)) & (who[nxt] == who[first])
                h2 = np.where(has_second, h[nxt], 256)
                o2 = np.where(has_second, octave[f][which[nxt]], -1)
                hb, ib = h[first], which[first]
                weak = hb > prm["max_hamming"]
                ratio = ~weak & (octave[f][ib] == o2) & (hb.astype(np.float64) > prm["nn_ratio"] * h2.astype(np.float64))
                good = ~weak & ~ratio
                ft[f, 6], ft[f, 7] = int(weak.sum()), int(ratio.sum())
                ft[f, 8] = int(good.sum())  # the proposals, until WON is known
                prop_node.append(f * cap + ib[good])
                prop_h.append(hb[good])
                prop_p.append(surv[who[first]][good])
            ft[f, 5] = len(surv) - len(first)
    row_dist = np.full(N, 0xFFFF, np.uint16)
    if c["row_point"] is not None:
        row_point, row_inlier = c["row_point"].astype(np.int32).copy(), (c["row_inlier"] != 0).astype(np.uint8)
    else:
        row_point = np.where(exists.reshape(-1), LOC_NO_POINT, LOC_NO_ROW).astype(np.int32)
        row_inlier = np.zeros(N, np.uint8)
    if prop_node:
        node, h, p = np.concatenate(prop_node), np.concatenate(prop_h), np.concatenate(prop_p)
        order = np.lexsort((p, h, node))
        node, h, p = node[order], h[order], p[order]
        win = np.flatnonzero(np.r_[True, node[1:] != node[:-1]]) if len(node) else np.zeros(0, np.int64)
        row_point[node[win]], row_inlier[node[win]], row_dist[node[win]] = p[win], 1, h[win]
        np.add.at(ft[:, 9], node[win] // cap, 1)
    ft[:, 8] -= ft[:, 9]
    totals = list(ft.sum(0)) + [len(searched), int(searchable.sum()) if len(searched) else 0]
    return dict(row_point=row_point, row_inlier=row_inlier, row_dist=row_dist, frame_totals=ft.astype(np.int32),
                totals=np.array(totals, np.int32))


def measure(ctx, name, n_search, repeats, host_repeats):
    import torch
    from gslam_amd import estimator, hip
    from localize_probe import CAP, CONFIGS, INLIER_THRESHOLD, INTRINSICS, N_FRAMES, N_NEW, RANSAC_THRESHOLD, SEED, median, stats, synth_map
    s = synth_map(CONFIGS[name])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(s[k]) for k in ("counts", "pair_q", "pair_t", "idx1", "keep", "node_point", "point_xyz", "status")}
    rng = np.random.default_rng(5)
    kps_host = s["kps"].copy()
    kps_host[..., 5] = rng.integers(0, 8, (N_FRAMES, CAP)).astype(np.int32).view(np.float32)
    d["kps"] = dev(kps_host)
    desc = dev(rng.integers(0, 256, (N_FRAMES, CAP, 32), dtype=np.uint8))
    N, P = N_FRAMES * CAP, len(s["point_xyz"])
    first_new = N_FRAMES - N_NEW
    poses_host = np.zeros((N_FRAMES, 7))
    poses_host[:, 3] = 1.0
    poses_host[:, 4:] = s["positions"]
    poses = dev(poses_host)
    # the map's observation list: one observation per mapped node
    nodes = torch.nonzero((d["node_point"] >= 0) & (d["node_point"] < P)).reshape(-1).to(torch.int32)
    obs_point = d["node_point"][nodes.long()].contiguous()
    obs_cam = (nodes // CAP).to(torch.int32).contiguous()
    summ = estimator.describe_points(ctx, d["kps"], desc, d["counts"], poses, obs_cam, obs_point, nodes.contiguous(), P, d["point_xyz"],
                                     point_status=d["status"])
    loc = estimator.localize_pairs(ctx, d["kps"], d["counts"], d["pair_q"], d["pair_t"], d["idx1"], d["keep"], d["node_point"],
                                   d["point_xyz"], d["status"], INTRINSICS, RANSAC_THRESHOLD, SEED, INLIER_THRESHOLD)
    poses[first_new:] = loc["poses"][first_new:]
    frame_search = torch.zeros(N_FRAMES, dtype=torch.uint8, device="cuda")
    frame_search[N_FRAMES - n_search:] = 1
    out = {"row_point": torch.empty(N, dtype=torch.int32, device="cuda"), "row_inlier": torch.empty(N, dtype=torch.uint8, device="cuda"),
           "row_dist": torch.empty(N, dtype=torch.uint16, device="cuda"),
           "frame_totals": torch.empty((N_FRAMES, 10), dtype=torch.int32, device="cuda"),
           "totals": torch.empty(12, dtype=torch.int32, device="cuda")}
    prm = estimator.search_default_params()
    pv = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None

    def search():
        ctx.check(hip.lib.gh_search_projection_dev(
            ctx.h, pv(d["kps"]), pv(desc), pv(d["counts"]), N_FRAMES, CAP, pv(poses), pv(frame_search), pv(d["node_point"]),
            pv(loc["row_point"]), pv(loc["row_inlier"]), P, pv(d["point_xyz"]), pv(d["status"]), None, pv(summ["point_views"]),
            pv(summ["point_desc"]), pv(summ["point_normal"]), pv(summ["point_dist"]), *(C.c_double(v) for v in INTRINSICS), SIZE[0],
            SIZE[1], C.byref(prm), *(pv(out[k]) for k in OUTPUTS)))
        torch.cuda.synchronize()

    call_us = median(search, repeats, 5)
    got = {k: out[k].cpu().numpy() for k in OUTPUTS}
    ctx.prof_enable(True)
    for _ in range(repeats):
        search()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    parts = {k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) for k in PARTS if k in prof}
    r = {"config": name, "device": ctx.device_info()["name"], "frames": N_FRAMES, "cap": CAP, "searched_frames": n_search, "nodes": N,
         "points": P, "totals": dict(zip(estimator.SEARCH_VERDICTS + ("searched", "searchable"), got["totals"].tolist())),
         "search_us": call_us, "search_parts_us": parts, "parts_sum_us": round(sum(parts.values()), 1)}
    if host_repeats > 0:
        params = {k: getattr(prm, k) for k, _ in hip.SearchParams._fields_}
        t_host, t_down, h = [], [], None
        for rep in range(host_repeats + 1):
            t0 = time.perf_counter()
            c = dict(kps=d["kps"].cpu().numpy(), desc=desc.cpu().numpy(), counts=d["counts"].cpu().numpy(), poses=poses.cpu().numpy(),
                     frame_search=frame_search.cpu().numpy(), node_point=d["node_point"].cpu().numpy(),
                     row_point=loc["row_point"].cpu().numpy(), row_inlier=loc["row_inlier"].cpu().numpy(), n_points=P,
                     xyz=d["point_xyz"].cpu().numpy(), status=d["status"].cpu().numpy(), select=None,
                     views=summ["point_views"].cpu().numpy(), point_desc=summ["point_desc"].cpu().numpy(),
                     normal=summ["point_normal"].cpu().numpy(), dist=summ["point_dist"].cpu().numpy(), intrinsics=INTRINSICS, size=SIZE)
            t1 = time.perf_counter()
            h = host_search(c, params)
            up = [dev(h[k]) for k in ("row_point", "row_inlier", "row_dist")]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:  # (the first run warms the allocator)
                t_down.append(t1 - t0)
                t_host.append(t2 - t0)
            del up
        same = {k: bool(h[k].tobytes() == got[k].tobytes()) for k in OUTPUTS}
        r.update({"host_download_us": stats(t_down), "host_route_us": stats(t_host),
                  "host_route_over_search": round(float(np.median(t_host)) * 1e6 / call_us["median"], 1),
                  "host_route_gives_the_same_arrays": all(same.values()), "host_route_same_by_array": same})
    return r


def main():
    import torch
    from gslam_amd import hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="map1")
    ap.add_argument("--searched", default="10,100")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--host-frames", type=int, default=10, help="the host route is run for the calls with at most this many frames")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    results = []
    for name in a.configs.split(","):
        for n in (int(v) for v in a.searched.split(",")):
            results.append(measure(ctx, name, n, a.repeats, a.host_repeats if n <= a.host_frames else 0))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/search_projection_probe.py: search by projection, gh_search_projection_dev (synthetic scene; medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
