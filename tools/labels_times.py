#!/usr/bin/env python3
"""What the softmax label units cost, 794 x 1024 (784 pixels + 10 labels), batch 4096, fp32 five-launch path, one MI355X:

  * us per kurbm_cd_step_labels against kurbm_cd_step on the same 794 plain columns (the same library with n_labels = 0: the
    launches of the step without the feature), alternating in one process after a common warm-up;
  * the label launch alone (kurbm_label_sample: by bytes it reads the 17 MB plane of h once);
  * kurbm_class_logits against ten kurbm_free_energy calls, the only road to the ten joint free energies -- and with them the
    class posterior -- without it.

Device events around `--calls` queued calls, the median of `--rounds` such windows.  Writes --out (default
profiles/labels_times.txt) and prints the same lines.  No pass / fail bar: these are first measurements."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_times.txt"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = np.random.default_rng(1)
W = g.normal(0, 0.05, (NV, NH)).astype(np.float32)
b_h, b_v = g.normal(0, 0.05, NH).astype(np.float32), g.normal(0, 0.05, NV).astype(np.float32)
pix = (g.random((B, NPIX)) < 0.19).astype(np.float32)
blk = np.zeros((B, C), np.float32)
blk[np.arange(B), g.integers(0, C, B)] = 1.0
V = DeviceMatrix.from_host(np.concatenate([pix, blk], axis=1), dev)
H = DeviceMatrix.from_host((g.random((B, NH)) < 0.5).astype(np.float32), dev)
e = DeviceRBM(W, b_h, b_v, dev)
ws_class = e.class_workspace(B)
state = {"step": 0}


def step(n_labels):
    # (lr = 0: the launches and their traffic are those of a training step, the parameters stay where they are)
    e.cd_step(V, B, 0, 0.0, 7, state["step"], n_labels=n_labels)
    state["step"] += 1


def ten_free_energies():
    for _ in range(C):
        e.free_energy(V, B)


variants = {
    "kurbm_cd_step (794 plain columns)": lambda: step(0),
    "kurbm_cd_step_labels (784 + 10)": lambda: step(C),
    "kurbm_label_sample alone": lambda: e.label_sample(H, V, C, 7, 1, 0),
    "kurbm_class_logits": lambda: e.class_logits(V, C, ws=ws_class),
    "10 x kurbm_free_energy": ten_free_energies,
}


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


for fn in variants.values():          # the common warm-up: code objects loaded, workspaces allocated
    window(fn, 5)
times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, fn in variants.items():
        times[name].append(window(fn, args.calls))
med = {name: statistics.median(ts) for name, ts in times.items()}
names = list(variants)
lines = ["softmax label units, %d x %d (%d pixels + %d labels), batch %d, fp32 five-launch path; %s" % (NV, NH, NPIX, C, B, torch.cuda.get_device_name(0)),
         "us per call: device events around %d queued calls, median of %d windows (all windows listed), variants alternating" % (args.calls, args.rounds)]
for name in names:
    lines.append("%-36s %8.1f us   (%s)" % (name, med[name], " ".join("%.1f" % x for x in times[name])))
lines.append("label units in a CD-1 step: %+.1f us = %+.1f %% of the plain step" % (med[names[1]] - med[names[0]], 100.0 * (med[names[1]] / med[names[0]] - 1.0)))
lines.append("class posterior: kurbm_class_logits is %.1f x faster than ten free energies" % (med[names[4]] / med[names[3]]))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
