"""Two-view initialisation of the frame pairs of one benchmark step, two ways.  Perf probe, not part of the product.

  batch      gh_two_view_batch_dev on 999 problems x 1200 rows, device-resident: one launch, ended by a synchronise.
  per pair   the only route without it: per pair a decomposition of E on the host (numpy SVD), four gh_triangulate calls
             (upload, launch, download and synchronise each), depth / reprojection tests and the vote on the host.  Timed
             on --subset pairs, scaled to 999.

Medians of repeated runs, after a warm-up.  The kernel time comes from gh_prof_* in a run of its own (event timing slows
the host side).  Prints one JSON object; --out FILE also writes it as text.

  python tools/two_view_probe.py --out profiles/two_view.txt"""
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


def rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quat(R):
    w = np.sqrt(max(1e-30, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2  # (the probe's rotations are far from pi)
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def median(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def host_route(ctx, E, src, dst, c2=0.99998 ** 2, r2=0.004 ** 2):
    """One pair without the batch entry -> (winner, good counts)."""
    U, _, Vt = np.linalg.svd(E.reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    d1, d2 = np.c_[src, np.ones(len(src))], np.c_[dst, np.ones(len(dst))]
    counts = []
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            X, ok = estimator.triangulate(ctx, np.r_[quat(R), t], d1, d2)
            Xc = X @ R.T + t
            with np.errstate(all="ignore"):
                a = d1 @ R.T
                cos2 = np.sum(a * d2, 1) ** 2 / (np.sum(a * a, 1) * np.sum(d2 * d2, 1))
                e1 = np.sum((X[:, :2] / X[:, 2:3] - src) ** 2, 1)
                e2 = np.sum((Xc[:, :2] / Xc[:, 2:3] - dst) ** 2, 1)
                good = ok & (X[:, 2] > 0) & (Xc[:, 2] > 0) & (cos2 < c2) & (e1 <= r2) & (e2 <= r2)
            counts.append(int(good.sum()))
    return int(np.argmax(counts)), counts


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=999)
    ap.add_argument("--rows", type=int, default=1200)
    ap.add_argument("--subset", type=int, default=40, help="pairs the per-pair route is timed on")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)

    rng = np.random.default_rng(1)
    R, t = rot([0.2, 1.0, 0.1], 0.12), np.array([0.6, 0.05, 0.1])
    X = np.c_[rng.uniform(-3, 3, (a.rows, 2)), rng.uniform(4, 9, a.rows)]
    X2 = X @ R.T + t
    src1 = X[:, :2] / X[:, 2:3]
    dst1 = X2[:, :2] / X2[:, 2:3] + rng.normal(size=(a.rows, 2)) * 2e-4
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E1 = np.r_[(tx @ R).reshape(9), 0, 0, 0]
    P = a.problems
    E = torch.from_numpy(np.tile(E1, (P, 1))).cuda()
    src = torch.from_numpy(np.tile(src1, (P, 1))).cuda()
    dst = torch.from_numpy(np.tile(dst1, (P, 1))).cuda()
    off = torch.arange(0, (P + 1) * a.rows, a.rows, dtype=torch.int32, device="cuda")
    prm = estimator.two_view_default_params()
    bufs = estimator.two_view_batch(ctx, E, src, dst, off, None, prm)  # (allocations outside the timed window)
    pv = lambda x: None if x is None else x.data_ptr()

    def batch():
        ctx.check(hip.lib.gh_two_view_batch_dev(ctx.h, pv(E), 12, pv(src), pv(dst), pv(off), P, None, C.byref(prm),
                                                *(pv(b) for b in bufs)))
        torch.cuda.synchronize()

    b_med, b_min, b_max = median(batch, a.repeats, 5)
    status = bufs[5].cpu().numpy()
    counts = bufs[3].cpu().numpy()
    assert (status == 0).all(), "the probe's problems are meant to come back OK"

    def per_pair():
        return host_route(ctx, E1[:9], src1, dst1)

    winner, hc = per_pair()
    # (numpy's SVD signs its vectors in its own way: the candidates come in another order, the support is the same)
    assert hc[winner] >= 0.99 * counts[0].max() and sorted(hc)[2] == 0, (hc, counts[0])
    p_med, p_min, p_max = median(per_pair, a.subset, 3)

    ctx.prof_enable(True)
    for _ in range(a.repeats):
        batch()
    prof = ctx.prof_collect().get("two_view", {"launches": 0, "total_ms": 0.0})
    ctx.prof_enable(False)
    out = {"device": ctx.device_info()["name"], "problems": P, "rows_per_problem": a.rows,
           "batch_call_us": {"median": round(b_med * 1e6, 1), "min": round(b_min * 1e6, 1), "max": round(b_max * 1e6, 1),
                             "repeats": a.repeats},
           "two_view_kernel_us": round(prof["total_ms"] * 1e3 / max(prof["launches"], 1), 1),
           "per_pair_route_us_per_pair": {"median": round(p_med * 1e6, 1), "min": round(p_min * 1e6, 1), "max": round(p_max * 1e6, 1),
                                          "pairs_timed": a.subset},
           "per_pair_route_us_scaled": round(p_med * 1e6 * P, 1),
           "speedup": round(p_med * P / b_med, 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/two_view_probe.py: two-view initialisation of %d pairs x %d rows (medians)\n" % (P, a.rows))
            for k, v in out.items():
                f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
