#!/usr/bin/env python3
"""us per temperature of an AIS run (kurbm_ais_run: two GEMM launches with beta in the epilogue and one small launch per
temperature, the whole schedule queued by ONE library call), 784 x 1024 with 512 and 4096 chains -- beside what one temperature
costs through the entry points the library had before: two fp32 half steps (v -> h, h -> v, Bernoulli draws) and two free-energy
calls (F at beta_{k-1} and at beta_k; each a softplus GEMM and its finish), queued back to back on preallocated buffers.  That sum
leaves out what the old route would also pay -- beta W rebuilt for every temperature and a host round trip for beta -- so it is a
floor for it.  One process, a common warm-up, the two alternating; device time between two events around the queued work.
Writes its lines to --out (default profiles/ais_times.txt) as well as to stdout."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd._lib import ACT_SIGMOID, NOISE_BERNOULLI, Rng, check  # noqa: E402
from keras_unsupervised_amd.ebm import ais  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM  # noqa: E402

NV, NH = 784, 1024

ap = argparse.ArgumentParser()
ap.add_argument("--temps", type=int, default=400, help="temperatures per timed run (>= 200)")
ap.add_argument("--rounds", type=int, default=5, help="timed runs per variant, alternating")
ap.add_argument("--chains", type=int, nargs="+", default=[512, 4096])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ais_times.txt"))
args = ap.parse_args()
assert args.temps >= 200

dev = torch.device("cuda", 0)
g = np.random.default_rng(0)
e = DeviceRBM(g.normal(0, 0.05, (NV, NH)).astype(np.float32), g.normal(0, 0.1, NH).astype(np.float32),
              g.normal(0, 0.1, NV).astype(np.float32), dev)
betas = ais.beta_schedule(args.temps)
lines = ["%s, %d x %d, %d temperatures per run, median of %d runs (us per temperature)"
         % (torch.cuda.get_device_name(0), NV, NH, args.temps, args.rounds)]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / args.temps


for M in args.chains:
    ws_ais = e.ais_workspace(M)
    b_a = e._base_bias(None)
    v = DeviceMatrix.from_host((torch.rand(M, NV, device=dev) < 0.3).float(), dev)
    h, v1 = DeviceMatrix.zeros(M, NH, dev), DeviceMatrix.zeros(M, NV, dev)
    F = torch.empty(M, dtype=torch.float32, device=dev)
    ws = e.workspace(M)
    lib, ctx, p, st = e.lib, e.ctx.handle, C.byref(e.params), e._stream()

    def native():
        e.ais_run(betas, M, base_bias=b_a, seed=1, ws=ws_ais)

    def existing():
        for k in range(1, args.temps + 1):
            rng = Rng(1, 0, 0x201, k)
            check(lib.kurbm_free_energy(ctx, p, v.ptr(), M, v.ld, F.data_ptr(), ws.data_ptr(), ws.numel(), st))
            check(lib.kurbm_free_energy(ctx, p, v.ptr(), M, v.ld, F.data_ptr(), ws.data_ptr(), ws.numel(), st))
            check(lib.kurbm_half_step_vh(ctx, p, v.ptr(), M, v.ld, ACT_SIGMOID, NOISE_BERNOULLI, C.byref(rng), h.ptr(), None, h.ld, st))
            check(lib.kurbm_half_step_hv(ctx, p, h.ptr(), M, h.ld, ACT_SIGMOID, NOISE_BERNOULLI, C.byref(rng), v1.ptr(), None, v1.ld, st))

    variants = {"kurbm_ais_run": native, "2 half steps + 2 free energies": existing}
    for fn in variants.values():      # the common warm-up: every kernel loaded, every buffer touched
        timed(fn)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    e.check_status()
    for name, ts in times.items():
        lines.append("%5d chains  %-32s %7.1f   (%s)" % (M, name, statistics.median(ts), " ".join("%.1f" % x for x in ts)))

print("\n".join(lines))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
