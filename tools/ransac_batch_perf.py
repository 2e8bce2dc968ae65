"""Geometric verification of the 999 consecutive frame pairs of a benchmark step: gh_ransac_batch_dev and
gh_ransac_pairs_dev against the loop of 999 gh_ransac_estimate calls that was the only way before them.

  python tools/ransac_batch_perf.py [--problems 999] [--rows 1000] [--cap 2000] [--reps 7] [--out FILE]

One context, seeded data, warm-up, medians of HIP-event and wall-clock times (the wall clock ends in a synchronise), the
ratio to the loop, a check that batch and loop return the same bytes, and the per-kernel split (gh_prof_*) from a run of
its own.  Needs a GPU."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gslam_amd import estimator, hip  # noqa: E402

SEED = 3


def two_view(rng, problems, rows, outliers=0.3, noise=0.2):
    """problems x rows pixel correspondences of a translating, slightly turning camera; a share of wrong matches."""
    X = np.concatenate([rng.uniform(-3, 3, (problems, rows, 2)), rng.uniform(4, 9, (problems, rows, 1))], axis=2)
    th = 0.1
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    X2 = X @ R.T + np.array([0.5, 0.05, 0.1])
    a = 500 * X[..., :2] / X[..., 2:3] + (320, 240)
    b = 500 * X2[..., :2] / X2[..., 2:3] + (320, 240) + rng.normal(size=a.shape) * noise
    bad = rng.random((problems, rows)) < outliers
    b[bad] = rng.uniform((0, 0), (640, 480), (int(bad.sum()), 2))
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def planar(rng, problems, rows, outliers=0.3, noise=0.3):
    a = rng.uniform((20, 20), (620, 460), (problems, rows, 2))
    H = np.array([[0.95, 0.04, 12.0], [-0.03, 1.02, -8.0], [2e-5, -1e-5, 1.0]])
    ah = np.concatenate([a, np.ones((problems, rows, 1))], axis=2) @ H.T
    b = ah[..., :2] / ah[..., 2:3] + rng.normal(size=a.shape) * noise
    bad = rng.random((problems, rows)) < outliers
    b[bad] = rng.uniform((0, 0), (640, 480), (int(bad.sum()), 2))
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def timed(fn, reps, warmup=2):
    """-> (median event ms, median wall ms) of fn(), which enqueues on torch's current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return statistics.median(ev), statistics.median(wall)


def loop_of_single_calls(ctx, model, src, dst, thr):
    """What a caller did before the batch: one gh_ransac_estimate per problem on host arrays.  -> (run, results)."""
    n, rows = src.shape[0], src.shape[1]
    models, masks, cnts = np.zeros((n, 12)), np.zeros((n, rows), np.uint8), np.zeros(n, np.int32)
    cnt = C.c_int()
    args = [(src[p].ctypes.data_as(C.c_void_p), dst[p].ctypes.data_as(C.c_void_p), models[p].ctypes.data_as(C.c_void_p),
             masks[p].ctypes.data_as(C.c_void_p)) for p in range(n)]
    fn, h, t, s = hip.lib.gh_ransac_estimate, ctx.h, C.c_double(thr), C.c_uint64(SEED)

    def run():
        for p, (a, b, m, k) in enumerate(args):
            st = fn(h, model, a, b, rows, t, s, m, k, C.byref(cnt))
            assert st == 0
            cnts[p] = cnt.value
    return run, (models, masks, cnts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=999)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ransac_batch_perf needs a GPU"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("ransac_batch_perf: %s, %d problems x %d rows, pair entry cap %d, %d repetitions (medians)" %
        (ctx.device_info()["name"], a.problems, a.rows, a.cap, a.reps))
    rng = np.random.default_rng(2024)
    for name, model, thr, make in (("H", estimator.HOMOGRAPHY, 2.0, planar), ("F", estimator.FUNDAMENTAL, 1.0, two_view)):
        src, dst = make(rng, a.problems, a.rows)
        d_src = torch.from_numpy(src.reshape(-1, 2)).cuda()
        d_dst = torch.from_numpy(dst.reshape(-1, 2)).cuda()
        off = torch.arange(0, (a.problems + 1) * a.rows, a.rows, dtype=torch.int32, device="cuda")
        out = {}

        def batch():
            out["r"] = estimator.estimate_batch(ctx, model, d_src, d_dst, off, thr, SEED)
        b_ev, b_wall = timed(batch, a.reps)
        run, (lm, lk, lc) = loop_of_single_calls(ctx, model, src, dst, thr)
        l_ev, l_wall = timed(run, max(3, a.reps // 2), warmup=1)
        bm, bk, bc = (t.cpu().numpy() for t in out["r"])
        same = bm.tobytes() == lm.tobytes() and bk.tobytes() == lk.tobytes() and bc.tobytes() == lc.tobytes()
        say("%s  batch %8.3f ms events %8.3f ms wall | loop of %d gh_ransac_estimate %8.3f ms wall (%.1f us per call) | "
            "loop / batch = %.1f | identical bytes: %s | mean inliers %.0f" %
            (name, b_ev, b_wall, a.problems, l_wall, l_wall * 1e3 / a.problems, l_wall / b_wall, same, bc.mean()))
        ctx.prof_enable(True)
        batch()
        torch.cuda.synchronize()
        for k, v in sorted(ctx.prof_collect().items()):
            say("     %-22s %3d launch(es) %9.3f ms" % (k, v["launches"], v["total_ms"]))
        ctx.prof_enable(False)

    # the pair entry on device-resident match rows: frames of one scene, consecutive pairs, row i matches row i
    F, cap = a.problems + 1, a.cap
    src, dst = two_view(rng, 1, cap, outliers=0.0, noise=0.0)
    kps = np.zeros((F, cap, 7), np.float32)
    step = (dst[0] - src[0])[None] * np.linspace(0, 1, F)[:, None, None]   # the scene drifts from the first view to the second
    kps[:, :, :2] = src[0][None] + step + rng.normal(size=(F, cap, 2)) * 0.2
    idx1 = np.tile(np.arange(cap, dtype=np.int32), (F - 1, 1))
    wrong = rng.random(idx1.shape) < 0.3
    idx1[wrong] = rng.integers(0, cap, int(wrong.sum()))
    keep = (rng.random(idx1.shape) < 0.5).astype(np.uint8)                   # about cap / 2 correspondences per pair
    d_kps, d_idx1, d_keep = torch.from_numpy(kps).cuda(), torch.from_numpy(idx1).cuda(), torch.from_numpy(keep).cuda()
    d_counts = torch.full((F,), cap, dtype=torch.int32, device="cuda")
    pq = torch.arange(0, F - 1, dtype=torch.int32, device="cuda")
    pt = pq + 1
    out = {}

    def pairs():
        out["r"] = estimator.estimate_pairs(ctx, estimator.FUNDAMENTAL, d_kps, d_counts, pq, pt, d_idx1, d_keep, 1.0, SEED)
    p_ev, p_wall = timed(pairs, a.reps)
    n_corr = out["r"][2].cpu().numpy()
    corr = estimator.correspondences_from_matches(kps[:3], np.full(3, cap), [0, 1], [1, 2], idx1[:2], keep[:2])
    single = [estimator.estimate(ctx, estimator.FUNDAMENTAL, s, d, 1.0, seed=SEED) for s, d, _ in corr]
    same = all(out["r"][0][p].cpu().numpy().tobytes() == single[p][0].tobytes() for p in range(2))
    say("F  pair entry, %d pairs, cap %d, %.0f correspondences per pair: %8.3f ms events %8.3f ms wall | first two pairs "
        "identical to gh_ransac_estimate: %s | mean inliers %.0f" %
        (F - 1, cap, n_corr.mean(), p_ev, p_wall, same, out["r"][3].float().mean().item()))
    ctx.prof_enable(True)
    pairs()
    torch.cuda.synchronize()
    for k, v in sorted(ctx.prof_collect().items()):
        say("     %-22s %3d launch(es) %9.3f ms" % (k, v["launches"], v["total_ms"]))
    ctx.prof_enable(False)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
