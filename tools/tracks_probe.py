"""Map-point creation from multi-view tracks (gh_triangulate_tracks_dev) on the graphs of BASELINE's C4 and C5.  Perf probe,
not part of the product.

  C4  500 cameras, 50 k points, 300 k observations      C5  10 k cameras, 1 M points, 6 M observations
  (ba_synth.make_graph: 6 observations per point, noise 0.002, 5 % outliers x50, the cameras at ground truth as after PnP;
  max_reproj 0.01, max_drops 2)

Per graph: the median of the whole call (device-resident, ended by a synchronise) after a warm-up; from gh_prof_* in a run of
its own (event timing slows the host side) the key kernel, the index build (rocPRIM sort + scan) and the triangulation kernel;
the round census (share of the OK points that went through 0 / 1 / 2 drops); the triangulation kernel against its byte floor
(24 B in and 1 B out per observation, 32 B out per point, the camera poses stay in cache) at 6.3 TB/s, the copy rate this
part reaches.  --skew N appends N more observations to point 0 of C4: one long track stalls its wave, the kernel waits for it.
Prints one JSON object per graph; --out FILE also writes them as text.

  python tools/tracks_probe.py --out profiles/tracks.txt"""
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
from gslam_amd.ba_synth import make_graph  # noqa: E402

HBM_COPY_RATE = 6.3e12  # bytes / s
CONFIGS = {"C4": (500, 50_000), "C5": (10_000, 1_000_000)}


def median(fn, n, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def measure(ctx, name, g, repeats, extra=None):
    import torch
    n_points = len(g["point_xyz"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cam, ocam, opt, oxy = dev(g["cam_pose"]), dev(g["obs_cam"]), dev(g["obs_point"]), dev(g["obs_xy"])
    n_obs = ocam.numel()
    prm = estimator.track_default_params()
    prm.max_reproj, prm.max_drops = 0.01, 2
    out = estimator.triangulate_tracks(ctx, cam, ocam, opt, oxy, n_points, params=prm)  # (allocations outside the timed window)
    pv = lambda x: C.c_void_p(x.data_ptr())

    def call():
        ctx.check(hip.lib.gh_triangulate_tracks_dev(ctx.h, pv(cam), cam.shape[0], pv(ocam), pv(opt), pv(oxy), n_obs, n_points, None, None,
                                                    C.byref(prm), *(pv(out[k]) for k in ("point_xyz", "status", "n_good", "obs_good"))))
        torch.cuda.synchronize()

    med, lo, hi = median(call, repeats, 5)
    ctx.prof_enable(True)
    for _ in range(repeats):
        call()
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    us = lambda k: round(prof[k]["total_ms"] * 1e3 / max(prof[k]["launches"], 1), 1) if k in prof else None
    status, n_good = out["status"].cpu().numpy(), out["n_good"].cpu().numpy()
    ok = status == 0
    per_point = np.bincount(g["obs_point"], minlength=n_points)
    drops = np.bincount((per_point[ok] - n_good[ok]).clip(0, 2), minlength=3)
    floor_bytes = 25 * n_obs + 32 * n_points
    floor_us = floor_bytes / HBM_COPY_RATE * 1e6
    res = {"graph": name, "device": ctx.device_info()["name"], "cameras": int(cam.shape[0]), "points": n_points, "observations": n_obs,
           "call_us": {"median": round(med * 1e6, 1), "min": round(lo * 1e6, 1), "max": round(hi * 1e6, 1), "repeats": repeats},
           "tracks_keys_us": us("tracks_keys"), "tracks_index_us": us("tracks_index"), "tracks_triangulate_us": us("tracks_triangulate"),
           "status_counts": np.bincount(status, minlength=6).tolist(),
           "drops_share_of_ok": [round(float(d) / max(int(ok.sum()), 1), 4) for d in drops],
           "triangulate_floor_bytes": floor_bytes, "triangulate_floor_us": round(floor_us, 1),
           "triangulate_fraction_of_floor": round(floor_us / us("tracks_triangulate"), 3) if us("tracks_triangulate") else None}
    if extra:
        res.update(extra)
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C4,C5")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skew", type=int, default=60_000, help="observations appended to point 0 of C4 (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    results = []
    for name in a.configs.split(","):
        n_cams, n_points = CONFIGS[name]
        g = make_graph(n_cams, n_points, 6, seed=1, perturb=False)
        results.append(measure(ctx, name, g, a.repeats))
        print(json.dumps(results[-1]), flush=True)
        if name == "C4" and a.skew > 0:
            first = np.flatnonzero(g["obs_point"] == 0)
            more = np.resize(first, a.skew)
            g2 = dict(g, obs_cam=np.r_[g["obs_cam"], g["obs_cam"][more]], obs_point=np.r_[g["obs_point"], g["obs_point"][more]],
                      obs_xy=np.r_[g["obs_xy"], g["obs_xy"][more]])
            results.append(measure(ctx, "C4 + one track of %d" % (a.skew + len(first)), g2, a.repeats, {"longest_track": int(a.skew + len(first))}))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/tracks_probe.py: map points from multi-view tracks, gh_triangulate_tracks_dev (medians; us)\n")
            for r in results:
                f.write("\n")
                for k, v in r.items():
                    f.write("%s: %s\n" % (k, json.dumps(v)))
    ctx.close()


if __name__ == "__main__":
    main()
