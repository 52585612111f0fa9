#!/usr/bin/env python3
"""us per sweep of a Gibbs run (kurbm_gibbs_run: the two x3 half-step launches per sweep on states that stay in their operand
format, the whole run queued by ONE library call), 784 x 1024 with 512 and 4096 chains, Bernoulli visibles, without a clamp and
with half of the visibles clamped -- beside the same number of sweeps through the public path the package had before:
inv_transform(transform(v)) in a Python loop on a device-resident matrix (two library calls, fresh fp32 planes and a conversion
back to the operand format per sweep).  One process, a common warm-up, the variants alternating; device time between two events
around the queued work, median of the rounds.
Writes its lines to --out (default profiles/gibbs_times.txt) as well as to stdout."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix  # noqa: E402

NV, NH = 784, 1024

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=400, help="sweeps per timed run (>= 200)")
ap.add_argument("--rounds", type=int, default=5, help="timed runs per variant, alternating")
ap.add_argument("--chains", type=int, nargs="+", default=[512, 4096])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gibbs_times.txt"))
args = ap.parse_args()
assert args.sweeps >= 200

dev = torch.device("cuda", 0)
g = np.random.default_rng(0)
weights = (g.normal(0, 0.05, (NV, NH)).astype(np.float32), g.normal(0, 0.1, NH).astype(np.float32),
           g.normal(0, 0.1, NV).astype(np.float32))
rbm = RBM({"batch_size": 512, "epochs": 1, "lr": 1e-3}, NH, mode=MODE_VISIBLE_BERNOULLI, seed=1, weights=weights, device=dev)
rbm.build((None, NV))
e = rbm._dev
half = torch.zeros(NV, dtype=torch.uint8, device=dev)
half[: NV // 2] = 1
lines = ["%s, %d x %d, Bernoulli visibles, %d sweeps per run, median of %d runs (us per sweep)"
         % (torch.cuda.get_device_name(0), NV, NH, args.sweeps, args.rounds)]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / args.sweeps


for M in args.chains:
    v = DeviceMatrix.from_host((torch.rand(M, NV, device=dev) < 0.3).float(), dev)
    v.bf16_exact = v.binary = True
    ws = e.gibbs_workspace(M, e._x3_pieces(v, None, MODE_VISIBLE_BERNOULLI), MODE_VISIBLE_BERNOULLI)

    def native(clamp=None):
        e.gibbs_run(v, burn_in=args.sweeps, chain0=0, seed=1, mode=MODE_VISIBLE_BERNOULLI, clamp=clamp, ws=ws)

    def public():
        x = v
        for _ in range(args.sweeps):
            x = rbm.inv_transform(rbm.transform(x))

    variants = {"kurbm_gibbs_run": native, "kurbm_gibbs_run, half clamped": lambda: native(half),
                "inv_transform(transform(v)) loop": public}
    for fn in variants.values():      # the common warm-up: every kernel loaded, every buffer touched
        timed(fn)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    e.check_status()
    for name, ts in times.items():
        lines.append("%5d chains  %-34s %7.1f   (%s)" % (M, name, statistics.median(ts), " ".join("%.1f" % x for x in ts)))

print("\n".join(lines))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
