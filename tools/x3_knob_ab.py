#!/usr/bin/env python3
"""A/B of one context knob in ONE process: the config-2 x3 CD-1 step (0/1 data, resident planes, as tools/x3_times.py times it) with
the knob at its two values alternating, HIP events around runs of 200 steps.

    python tools/x3_knob_ab.py [KNOB [A B [PAIRS]]]        default: KURBM_X3_PACKED_EPI 1 0 6

Prints every run, then the medians.  The knob is left at A."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd._lib import Context  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM  # noqa: E402

knob = sys.argv[1] if len(sys.argv) > 1 else "KURBM_X3_PACKED_EPI"
va, vb = (int(x) for x in sys.argv[2:4]) if len(sys.argv) > 3 else (1, 0)
pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 6
B, NV, NH = 4096, 784, 1024
dev = torch.device("cuda", 0)
g = np.random.default_rng(1)
eng = DeviceRBM(g.uniform(-0.05, 0.05, (NV, NH)).astype(np.float32), np.zeros(NH, np.float32), np.zeros(NV, np.float32), dev)
V = DeviceMatrix.from_host((g.random((B, NV)) < 0.19).astype(np.float32), dev)
planes = eng.make_planes(V, [(0, B)])
ctx = Context.get(dev.index)


def run(iters=200):
    for i in range(20):
        eng.cd_step(V, B, 0, 1e-3 / B, 42, i, compute="x3", planes=planes)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        eng.cd_step(V, B, 0, 1e-3 / B, 42, 20 + i, compute="x3", planes=planes)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


res = {va: [], vb: []}
try:
    for p in range(pairs):
        for val in (va, vb):
            ctx.set_option(knob, val)
            res[val].append(run())
            print("pair %d  %s=%d  %7.2f us / step" % (p, knob, val, res[val][-1]), flush=True)
finally:
    ctx.set_option(knob, va)
ma, mb = np.median(res[va]), np.median(res[vb])
print("%s=%d median %.2f us (min %.2f max %.2f) | =%d median %.2f us (min %.2f max %.2f) | %d - %d: %+.2f us"
      % (knob, va, ma, min(res[va]), max(res[va]), vb, mb, min(res[vb]), max(res[vb]), va, vb, ma - mb))
