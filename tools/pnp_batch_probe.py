"""Pose refinement of the tracked frames of one benchmark sequence, two ways.  Perf probe, not part of the product.

  batch      gh_pnp_refine_batch_dev on 999 problems x 300 rows (10 % gross outliers, default options), device-resident:
             one launch, ended by a synchronise.
  kernel     the same launch timed by gh_prof_* events, in a run of its own (event timing slows the host side).
  loop       the route it replaces: gh_ba_pnp once per problem on host arrays (upload, launch, download and a stream
             synchronise each).
  by rows    the kernel alone at 64 .. 1024 rows per problem.  The kernel is a part that does not depend on the rows (the 6 x 6
             solve on thread 0, the block sums and their barriers) plus row passes of ceil(rows / 256) trips: the times at 256,
             512, 768 and 1024 rows differ by whole trips, so their slope is one trip of every pass and what is left of the
             256-row time is the row-independent part.

Medians of repeated runs, after a warm-up, with their ranges.  Prints one JSON object; --out FILE also writes it as text.

  python tools/pnp_batch_probe.py --out profiles/pnp_batch.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gslam_amd import ba, estimator, hip  # noqa: E402
from gslam_amd.ba_synth import make_graph  # noqa: E402


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"median": round(float(np.median(t)) * 1e6, 1), "min": round(min(t) * 1e6, 1), "max": round(max(t) * 1e6, 1), "repeats": n}


def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def problem(rows, seed=41):
    """One tracked frame: `rows` 3D-2D matches of camera 1 of a small graph, noise 0.002, every tenth observation a gross
    outlier, the start a few centimetres and degrees off the truth."""
    g = make_graph(3, rows, n_obs_per_point=3, seed=seed, noise=0.0, outlier_frac=0.0, perturb=False)
    sel = g["obs_cam"] == 1
    X = np.ascontiguousarray(g["point_xyz_gt"][g["obs_point"][sel]])
    rng = np.random.default_rng(seed)
    m = g["obs_xy"][sel] + rng.standard_normal((len(X), 2)) * 0.002
    m[::10] += rng.standard_normal((len(m[::10]), 2)) * 0.1
    pose = g["cam_pose_gt"][1].copy()
    w = np.array([0.01, -0.02, 0.015])
    q = qmul(pose[:4], np.r_[0.5 * w, 1.0])
    pose[:4] = q / np.linalg.norm(q)
    pose[4:] += [0.05, -0.04, 0.03]
    return X, np.ascontiguousarray(m), pose


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=999)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    P = a.problems
    opt = ba.default_options()
    pv = lambda x: None if x is None else x.data_ptr()

    def setup(rows):
        X1, m1, start1 = problem(rows)
        xyz = torch.from_numpy(np.tile(X1, (P, 1))).cuda()
        xy = torch.from_numpy(np.tile(m1, (P, 1))).cuda()
        start = torch.from_numpy(np.tile(start1, (P, 1))).cuda()
        off = torch.arange(0, (P + 1) * rows, rows, dtype=torch.int32, device="cuda")
        bufs = estimator.pnp_refine_batch(ctx, xyz, xy, off, start, options=opt, inlier_threshold=0.006, want_information=True)
        order = ("poses", "info", "summaries", "inlier", "n_inliers")  # (allocations outside the timed window)

        def batch():
            ctx.check(hip.lib.gh_pnp_refine_batch_dev(ctx.h, pv(xyz), pv(xy), pv(off), P, P * rows, None, pv(start), 7, 63, C.byref(opt),
                                                      0, C.c_double(0.006), *(pv(bufs[k]) for k in order)))
            torch.cuda.synchronize()
        return X1, m1, start1, bufs, batch

    def kernel_us(batch, n):
        ctx.prof_enable(True)
        for _ in range(n):
            batch()
        prof = ctx.prof_collect().get("pnp_refine_batch", {"launches": 0, "total_ms": 0.0})
        ctx.prof_enable(False)
        return round(prof["total_ms"] * 1e3 / max(prof["launches"], 1), 1)

    X1, m1, start1, bufs, batch = setup(a.rows)
    call = timed(batch, a.repeats, 5)
    sums = bufs["summaries"].cpu().numpy().view(estimator.SUMMARY_DTYPE).reshape(P)
    assert (sums["termination"] <= 2).all() and (sums["final_cost"] < sums["initial_cost"]).all(), "the probe's problems are meant to converge"
    pose1, s1, _ = ba.pnp(ctx, X1, m1, start1, options=opt, want_information=True)
    assert bufs["poses"][0].cpu().numpy().tobytes() == pose1.tobytes(), "the batch is meant to equal the single call"

    def loop():
        for _ in range(P):
            ba.pnp(ctx, X1, m1, start1, options=opt, want_information=True)

    lp = timed(loop, a.repeats, 2)
    kern = kernel_us(batch, a.repeats)

    by_rows = {}
    for rows in (64, 256, 512, 768, 1024):
        _, _, _, b, fn = setup(rows)
        fn()
        it = b["summaries"].cpu().numpy().view(estimator.SUMMARY_DTYPE)["iterations"]
        by_rows[str(rows)] = {"kernel_us": kernel_us(fn, 10), "iterations": int(it.reshape(-1)[0])}
    # 256 -> 1024 rows adds three whole trips to every row pass: the slope is a trip of all passes, the rest of the 256-row
    # time does not depend on the rows (the solve on thread 0, the block sums and their barriers, the launch)
    split = None
    if len({by_rows[r]["iterations"] for r in ("256", "512", "768", "1024")}) == 1:
        trip = (by_rows["1024"]["kernel_us"] - by_rows["256"]["kernel_us"]) / 3.0
        split = {"kernel_us_at_256_rows": by_rows["256"]["kernel_us"], "one_trip_of_every_row_pass_us": round(trip, 1),
                 "row_independent_us": round(by_rows["256"]["kernel_us"] - trip, 1)}

    out = {"device": ctx.device_info()["name"], "problems": P, "rows_per_problem": a.rows, "outliers": "every 10th row",
           "iterations_per_problem": int(s1.iterations),
           "batch_call_us": call, "refine_kernel_us": kern, "loop_of_gh_ba_pnp_us": lp,
           "loop_us_per_problem": round(lp["median"] / P, 2), "speedup_loop_over_batch": round(lp["median"] / call["median"], 1),
           "kernel_by_rows": by_rows, "split_at_256_rows": split}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/pnp_batch_probe.py: pose refinement of %d problems x %d rows (medians, ranges)\n" % (P, a.rows))
            for k, v in out.items():
                f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
