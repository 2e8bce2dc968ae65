#!/usr/bin/env python3
"""What low-texture video pays for the two-phase FAST detector: ORB extraction time per call on 1080p batches where the
second phase (orb_select redoing the cells without a strong corner) carries the load.

  low_contrast  every cell weak: all scores sit between min_th and ini_th (tests/orb_images.py); nothing passes the compass test
                at ini_th, so fast_cells finishes every tile single-phase
  few_corners   flat background with 12 bright squares per frame: nearly every tile flat
  weak_tiles    30 % of the pixels 12 above the others (every score is 12) and ONE corner of score 100 in every 64 x 64 tile: no
                tile can be finished single-phase and three cells of four are left to orb_select -- the input on which the second
                phase carries the most

    python tools/orb_two_phase_worst.py [frames]           (GSLAM_HIP_LIB=<other build> for the other side of an A/B)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from gslam_amd import hip
from gslam_amd.orb import OrbExtractor
from orb_images import CLASSES

W, H, K = 1920, 1080, 2000


def weak_tiles(w, h, seed):
    img = np.where(np.random.default_rng(seed).random((h, w)) < 0.3, 112, 100).astype(np.uint8)
    for y in range(19 + 10, h - 19, 64):
        for x in range(19 + 10, w - 19, 64):
            img[y - 4:y + 5, x - 4:x + 5] = 100
            img[y, x] = 200
    return img


GENERATORS = {"low_contrast": CLASSES["low_contrast"], "few_corners": CLASSES["few_corners"], "weak_tiles": weak_tiles}
B = int(sys.argv[1]) if len(sys.argv) > 1 else 300
DISTINCT = 12
ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ex = OrbExtractor(ctx, W, H, max_batch=B, n_features=K)
print("library", hip.LIB_PATH)
for name in GENERATORS:
    base = np.stack([GENERATORS[name](W, H, 700 + i) for i in range(DISTINCT)])
    fr = torch.from_numpy(base).cuda()[torch.arange(B) % DISTINCT].contiguous()
    out = ex.alloc_outputs(B)
    ex.extract(fr, out)
    torch.cuda.synchronize()
    ms = []
    for rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ex.extract(fr, out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print("%-13s %d x %dx%d: %.3f ms per call (min of 5; all: %s), %d keypoints" %
          (name, B, W, H, min(ms), " ".join("%.3f" % m for m in ms), int(out[2].sum())))
    ctx.prof_enable(True)
    ex.extract(fr, out)
    for k, v in ctx.prof_collect().items():
        print("    %-18s launches %3d  total %.3f ms" % (k, v["launches"], v["total_ms"]))
    ctx.prof_enable(False)
    del fr, out
