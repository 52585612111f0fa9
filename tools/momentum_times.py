#!/usr/bin/env python3
"""What momentum and weight decay cost: us per step of the quiet x3 loop (fit(verbose=0): every batch of an epoch queued by one
library call), 784 x 1024, batch 4096, 0/1 data -- the bare rule against momentum 0.9 + weight decay, in ONE process after a
common warm-up, the two alternating (boxes differ by ~5 %, and the loops are clock-limited: only the plain step of the same run
is a fair yardstick).  The velocity adds one 16-byte load and store per weight group to the launch that reduces the slabs and
rewrites the weights and their bf16 pieces (k_reduce_apply_split -> k_reduce_apply_split_mom): 6.4 MB on top of ~30 MB.
Same protocol as tools/score_times.py.  --json PATH also writes the numbers there.  For the per-launch time of the two reduce
kernels run this file under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix  # noqa: E402

N, NV, NH, B = 65536, 784, 1024, 4096

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=4, help="epochs (of 16 steps) per timed fit")
ap.add_argument("--rounds", type=int, default=5, help="timed fits per variant, alternating")
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
V = DeviceMatrix.from_host((torch.rand(N, NV, device=dev) < 0.19).float(), dev)
hps = {"batch_size": B, "epochs": 1, "lr": 1e-3 / B}
variants = {"plain": RBM(dict(hps), NH, mode=MODE_VISIBLE_BERNOULLI, seed=1, compute_dtype="x3"),
            # (weight_decay on the scale of the batch sums: Hinton's 1e-4 per case times the batch size)
            "momentum": RBM(dict(hps, momentum=0.9, weight_decay=1e-4 * B), NH, mode=MODE_VISIBLE_BERNOULLI, seed=1, compute_dtype="x3")}


def fit_us_per_step(r, epochs):
    r.hps["epochs"] = epochs
    t0 = time.perf_counter()
    r.fit(V, verbose=0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (epochs * (N // B)) * 1e6


for r in variants.values():           # the common warm-up: both code paths loaded, both mirrors and workspaces allocated
    r.build((None, NV))
    fit_us_per_step(r, 1)
times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, r in variants.items():
        times[name].append(fit_us_per_step(r, args.epochs))
med = {name: statistics.median(ts) for name, ts in times.items()}
for name, ts in times.items():
    print("%-9s fit(verbose=0) %.1f us/step (median of %d fits of %d steps; %s)"
          % (name, med[name], len(ts), args.epochs * (N // B), " ".join("%.1f" % x for x in ts)))
print("momentum + weight decay: %+.1f us/step = %+.1f %%" % (med["momentum"] - med["plain"], 100.0 * (med["momentum"] / med["plain"] - 1.0)))
if args.json:
    with open(args.json, "w") as f:
        json.dump({"shape": [NV, NH], "batch": B, "steps_per_fit": args.epochs * (N // B), "us_per_step": times, "median_us_per_step": med,
                   "device": torch.cuda.get_device_name(0)}, f, indent=1)
