#!/usr/bin/env python3
"""What discriminative and hybrid training of a label RBM cost, 794 x 1024 (784 pixels + 10 labels), batch 4096, fp32 path, one
MI355X:

  * us for k_class_grad alone, and for the launches in front of it and behind it (the measurement knob KURBM_DISC_STAGE makes
    kurbm_class_grad run one group of its launches on the planes a complete call left in the workspace);
  * us per kurbm_disc_step with gen_weight = 0 (discriminative) and gen_weight = 0.01 (hybrid);
  * us per kurbm_cd_step_labels on the same data, the generative step the two are compared with.

Device events around `--calls` queued calls, the median of `--rounds` such windows, variants alternating after a common warm-up.
Writes --out (default profiles/disc_times.txt) and prints the same lines.  No pass / fail bar: these are first measurements."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM  # noqa: E402

NPIX, C, NH, B = 784, 10, 1024, 4096
NV = NPIX + C

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50, help="queued calls per timed window")
ap.add_argument("--rounds", type=int, default=7, help="timed windows per variant, alternating")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_times.txt"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = np.random.default_rng(1)
W = g.normal(0, 0.05, (NV, NH)).astype(np.float32)
b_h, b_v = g.normal(0, 0.05, NH).astype(np.float32), g.normal(0, 0.05, NV).astype(np.float32)
pix = (g.random((B, NPIX)) < 0.19).astype(np.float32)
blk = np.zeros((B, C), np.float32)
blk[np.arange(B), g.integers(0, C, B)] = 1.0
V = DeviceMatrix.from_host(np.concatenate([pix, blk], axis=1), dev)
e = DeviceRBM(W, b_h, b_v, dev)
ws = e.disc_workspace(B, C, V.ld)
state = {"step": 0}


def hook(stage):
    e.ctx.set_option("KURBM_DISC_STAGE", stage)
    e.class_grad(V, C, want_planes=False, want_nll=False, ws=ws)
    e.ctx.set_option("KURBM_DISC_STAGE", 0)


def disc(gen_weight):
    # (lr = 0: the launches and their traffic are those of a training step, the parameters stay where they are)
    e.disc_step(V, B, 0, 0.0, C, gen_weight=gen_weight, seed=7, step=state["step"], ws=ws)
    state["step"] += 1


def cd_labels():
    e.cd_step(V, B, 0, 0.0, 7, state["step"], n_labels=C)
    state["step"] += 1


variants = {
    "k_class_grad alone": lambda: hook(2),
    "half step + k_class_logits": lambda: hook(1),
    "statistics GEMM + reductions": lambda: hook(3),
    "kurbm_class_grad (all of the above)": lambda: hook(0),
    "kurbm_disc_step, gen_weight = 0": lambda: disc(0.0),
    "kurbm_disc_step, gen_weight = 0.01": lambda: disc(0.01),
    "kurbm_cd_step_labels (784 + 10)": cd_labels,
}


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


hook(0)                               # a complete call: the planes the staged calls run on
for fn in variants.values():          # the common warm-up: code objects loaded, workspaces allocated
    window(fn, 5)
times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, fn in variants.items():
        times[name].append(window(fn, args.calls))
med = {name: statistics.median(ts) for name, ts in times.items()}
names = list(variants)
sigmoids = B * NH * C
planes_mb = 2 * B * NH * 4 / 1e6     # a read, g written (S_y and H_bar leave only for the test hook)
lines = ["discriminative / hybrid training, %d x %d (%d pixels + %d labels), batch %d, fp32 path; %s" % (NV, NH, NPIX, C, B, torch.cuda.get_device_name(0)),
         "us per call: device events around %d queued calls, median of %d windows (all windows listed), variants alternating" % (args.calls, args.rounds)]
for name in names:
    lines.append("%-38s %8.1f us   (%s)" % (name, med[name], " ".join("%.1f" % x for x in times[name])))
t_cg = med[names[0]]
lines.append("k_class_grad: %.1f M sigmoids and %.1f MB of planes in %.1f us = %.2f G sigmoid/s, %.2f TB/s"
             % (sigmoids / 1e6, planes_mb, t_cg, sigmoids / t_cg / 1e3, planes_mb / t_cg))
lines.append("discriminative step against the CD-1 label step: %+.1f us = %+.1f %%" % (med[names[4]] - med[names[6]], 100.0 * (med[names[4]] / med[names[6]] - 1.0)))
lines.append("hybrid step against their sum: %+.1f us (no apply is saved: the label step's apply is fused into its slab reduction, which still runs"
             % (med[names[5]] - med[names[4]] - med[names[6]]))
lines.append("  to emit its delta, and k_class_reduce adds gen_weight x that delta in one more pass over the packed delta)")
lines.append("k_class_grad against the statistics GEMM + reductions: %.2f x" % (med[names[0]] / med[names[2]]))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
