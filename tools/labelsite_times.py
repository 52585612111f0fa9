#!/usr/bin/env python3
"""What a free label block costs in the Gibbs and AIS runs: a 784 + 10 -> 1024 label RBM with 512 and 4096 chains on one MI355X
(include/kurbm.h, "free label blocks").

  * us per Gibbs sweep with a free block (kurbm_gibbs_run_labels) against the same run with the block clamped through
    kurbm_gibbs_run -- the path a label RBM had before -- and against the unclamped plain run (no site, no clamp launch: the block
    sampled as Bernoulli units, a timing yardstick only).  free - unclamped = the site's own launch; clamped - unclamped = the clamp
    launch it stands beside;
  * us per AIS temperature with labels (kurbm_ais_run_labels) against kurbm_ais_run on the same 794 plain columns; the difference is
    the site's launch less the ten columns the h -> v launch no longer covers.

Device events around one queued run of --sweeps sweeps / temperatures, the median of --rounds such windows, variants alternating
after a common warm-up.  Writes --out (default profiles/labelsite_times.txt) and prints the same lines.  No pass / fail bar: these
are first measurements."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd.ebm import ais  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM  # noqa: E402

NPIX, C, NH = 784, 10, 1024
NV = NPIX + C

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=200, help="Gibbs sweeps / AIS temperatures per timed run")
ap.add_argument("--rounds", type=int, default=7, help="timed windows per variant, alternating")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labelsite_times.txt"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = np.random.default_rng(1)
eng = DeviceRBM(g.normal(0, 0.05, (NV, NH)).astype(np.float32), g.normal(0, 0.05, NH).astype(np.float32),
                g.normal(0, 0.05, NV).astype(np.float32), dev)
b_a = g.normal(0, 0.3, NV).astype(np.float32)
betas = ais.beta_schedule(args.sweeps)
block = np.zeros(NV, dtype=bool)
block[NPIX:] = True


def window(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / args.sweeps


lines = ["free label blocks, %d + %d -> %d; %s" % (NPIX, C, NH, torch.cuda.get_device_name(0)),
         "us per sweep / temperature: device events around one queued run of %d, median of %d windows (all listed), variants alternating"
         % (args.sweeps, args.rounds)]
for rows in (512, 4096):
    pix = (g.random((rows, NPIX)) < 0.19).astype(np.float32)
    blk = np.zeros((rows, C), np.float32)
    blk[np.arange(rows), g.integers(0, C, rows)] = 1.0
    v0 = DeviceMatrix.from_host(np.concatenate([pix, blk], axis=1), dev)
    v0.bf16_exact = v0.binary = True
    gws = eng.gibbs_workspace(rows, 1 | 0x10, 0)
    aws, awsl = eng.ais_workspace(rows), eng.ais_workspace(rows, C)
    mask = eng._clamp_mask(block)
    variants = {
        "Gibbs sweep, free block (kurbm_gibbs_run_labels)": lambda: eng.gibbs_run(v0, burn_in=args.sweeps, seed=3, ws=gws, n_labels=C),
        "Gibbs sweep, block clamped (kurbm_gibbs_run)": lambda: eng.gibbs_run(v0, burn_in=args.sweeps, seed=3, ws=gws, clamp=mask),
        "Gibbs sweep, no site and no clamp (yardstick)": lambda: eng.gibbs_run(v0, burn_in=args.sweeps, seed=3, ws=gws),
        "AIS temperature, labels (kurbm_ais_run_labels)": lambda: eng.ais_run(betas, rows, base_bias=b_a, seed=3, ws=awsl, n_labels=C),
        "AIS temperature, 794 plain columns (kurbm_ais_run)": lambda: eng.ais_run(betas, rows, base_bias=b_a, seed=3, ws=aws),
    }
    for fn in variants.values():          # the common warm-up: code objects loaded, buffers allocated
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(window(fn))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    names = list(variants)
    lines.append("%d chains" % rows)
    for name in names:
        lines.append("  %-52s %8.2f us   (%s)" % (name, med[name], " ".join("%.2f" % x for x in times[name])))
    lines.append("  the Gibbs site's own launch (free - yardstick): %.2f us; the clamp launch (clamped - yardstick): %.2f us"
                 % (med[names[0]] - med[names[2]], med[names[1]] - med[names[2]]))
    lines.append("  the AIS site's launch less ten columns of the h -> v launch (labels - plain): %.2f us" % (med[names[3]] - med[names[4]]))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
