#!/usr/bin/env python3
"""What the threshold hint of large ORB calls (gh_orb_plan_set_threshold_hint) pays when its advice is wrong: ORB extraction
time per call over 200 calls on ONE plan of 300 x 1080p, hints on (adaptive) against hints off, on

  steady       the same textured batch every call: the advice holds from the second call on
  alternating  a textured batch and the same frames at a quarter of the contrast, alternating every call: every slot's advice
               from the textured call is wrong for the next one
  permuted     a batch of textured, quarter-contrast and flat frames, permuted between the slots every call

A misprediction costs the level redone by one orb_select workgroup; the hold-off keeps a slot that mispredicted at ini_th for
2, 4, .. 64 calls.  `redo` below is the cost of redoing EVERY level of EVERY slot in one call (forced T = 255 against hints off).

    python tools/orb_hint_mispredict.py [frames] [calls]     (GSLAM_HIP_LIB=<other build> for the other side of an A/B)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gslam_amd import hip
from gslam_amd.orb import OrbExtractor, synth_frames

W, H, K = 1920, 1080, 2000
B = int(sys.argv[1]) if len(sys.argv) > 1 else 300
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ctx = hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
print("library", hip.LIB_PATH)

textured = synth_frames(ctx, B, W, H)
quarter = (textured >> 2) + 96          # the same corners at a quarter of their scores
mixed = textured.clone()
mixed[1::3] = quarter[1::3]
mixed[2::3] = 100
gen = torch.Generator(device="cpu").manual_seed(7)
perms = [torch.randperm(B, generator=gen).cuda() for _ in range(CALLS)]


def batches(name):
    """call index -> the batch of that call"""
    if name == "steady":
        return lambda i: textured
    if name == "alternating":
        return lambda i: textured if i % 2 == 0 else quarter
    buf = [torch.empty_like(mixed), torch.empty_like(mixed)]

    def permuted(i):
        torch.index_select(mixed, 0, perms[i], out=buf[i & 1])
        return buf[i & 1]
    return permuted


def run(name, mode, value=0, calls=CALLS):
    ex = OrbExtractor(ctx, W, H, max_batch=B, n_features=K)
    ex.threshold_hint(mode, value)
    out = ex.alloc_outputs(B)
    get = batches(name)
    ms = []
    for i in range(calls):
        fr = get(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ex.extract(fr, out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    hints = ex.debug_hints() if mode == "adaptive" else None
    ex.close()
    return np.array(ms), hints, int(out[2].sum())


for name in ("steady", "alternating", "permuted"):
    res = {}
    for arm, mode in (("off", "off"), ("on", "adaptive"), ("off2", "off"), ("on2", "adaptive")):
        ms, hints, n = run(name, mode)
        res[arm] = ms
        print("%-12s hints %-4s %d calls of %d x %dx%d: mean %.3f ms, median %.3f, min %.3f, max %.3f (calls 2..: mean %.3f)%s" %
              (name, arm, len(ms), B, W, H, ms.mean(), np.median(ms), ms.min(), ms.max(), ms[2:].mean(),
               "" if hints is None else ", slots above ini_th at the end: %d of %d" % (int((hints > 20).sum()), hints.size)))
    off = np.concatenate([res["off"][2:], res["off2"][2:]]).mean()
    on = np.concatenate([res["on"][2:], res["on2"][2:]]).mean()
    spread = abs(res["off"][2:].mean() - res["off2"][2:].mean())
    print("%-12s amortised on - off: %+.3f ms per call (off %.3f, on %.3f; the two off runs differ by %.3f); slowest 5 calls with "
          "hints on: %s" % (name, on - off, off, on, spread, " ".join("%d:%.2f" % (i, res["on"][i]) for i in np.argsort(res["on"])[-5:][::-1])))

base, _, _ = run("steady", "off", calls=6)
redo, _, _ = run("steady", "forced", 255, calls=6)
print("redo: every level of every slot redone in one call: %.3f ms against %.3f ms with hints off -> %.3f ms per call; a slot "
      "that mispredicts at every chance is redone once in 66 calls, %.3f ms per call amortised if ALL %d slots do" %
      (np.median(redo[1:]), np.median(base[1:]), np.median(redo[1:]) - np.median(base[1:]),
       (np.median(redo[1:]) - np.median(base[1:])) / 66, B))
