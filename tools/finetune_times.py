#!/usr/bin/env python3
"""What a fine-tuning step of a DBN costs: 784 -> 1024 -> 1024 under a 1024 + 10 -> 1024 label RBM, batch 4096, fp32 path, one
MI355X (DBN.fine_tune; include/kurbm.h, "fine-tuning a DBN").

  * us per step -- the calls DBN.fine_tune makes for one batch, lr = 0 -- and per launch group: the forward half steps, the top
    layer's kurbm_disc_backprop, each lower layer's kurbm_backprop_layer, the three applies;
  * yardstick (a): k_backprop_delta + k_backprop_reduce (kurbm_backprop_delta, out of place: e and x read, delta written) against a
    device-to-device copy that moves the same bytes -- 1.5 planes copied = 3 planes of traffic;
  * yardstick (b): the step against the sum of the EXISTING calls it is made of -- the top's kurbm_class_grad; per lower layer one
    prob-only v -> h half step, one linear h -> v half step (layer 2 only: the bottom layer needs no e_in) and one one-segment
    statistics GEMM with its reductions (KURBM_DISC_STAGE = 3 of kurbm_class_grad on a label RBM with that many pixel rows: the same
    GEMM and slab reduction, k_class_reduce in k_backprop_reduce's place); the applies -- plus (a) once per lower layer.

Device events around `--calls` queued calls, the median of `--rounds` such windows, variants alternating after a common warm-up
(the protocol of tools/disc_times.py).  Writes --out (default profiles/finetune_times.txt) and prints the same lines.  No pass /
fail bar: these are first measurements."""
import argparse
import ctypes as C_
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keras_unsupervised_amd._lib import ACT_LINEAR, ACT_SIGMOID, NOISE_NONE, check  # noqa: E402
from keras_unsupervised_amd.ebm.engine import DeviceMatrix, DeviceRBM  # noqa: E402

N0, N1, N2, C, NT, B = 784, 1024, 1024, 10, 1024, 4096

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50, help="queued calls per timed window")
ap.add_argument("--rounds", type=int, default=7, help="timed windows per variant, alternating")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_times.txt"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = np.random.default_rng(1)
rbm = lambda nv, nh: DeviceRBM(g.normal(0, 0.05, (nv, nh)).astype(np.float32), g.normal(0, 0.05, nh).astype(np.float32),
                               g.normal(0, 0.05, nv).astype(np.float32), dev)
l1, l2, top = rbm(N0, N1), rbm(N1, N2), rbm(N2 + C, NT)
aux1 = rbm(N0 + C, N1)       # a label RBM with layer 1's pixel rows: its KURBM_DISC_STAGE = 3 is layer 1's statistics GEMM + reductions
pix = (g.random((B, N0)) < 0.19).astype(np.float32)
blk = np.zeros((B, C), np.float32)
blk[np.arange(B), g.integers(0, C, B)] = 1.0
V = DeviceMatrix.from_host(pix, dev)
VL = DeviceMatrix.from_host(np.concatenate([pix, blk], axis=1), dev)
onehot = torch.from_numpy(blk).to(dev)
x1, plane = DeviceMatrix.zeros(B, N1, dev), DeviceMatrix.zeros(B, N2 + C, dev)
e1, e2 = DeviceMatrix.zeros(B, N1, dev), DeviceMatrix.zeros(B, N2, dev)
xs_site, es_site = DeviceMatrix.zeros(B, N1, dev), DeviceMatrix.zeros(B, N1, dev)
xs_site.t.uniform_(0.05, 0.95)
es_site.t.normal_()
ws_site = l1.backprop_workspace(B, 1)
half = torch.empty(3 * B * N1 * 4, dtype=torch.uint8, device=dev)             # two halves of 1.5 fp32 planes each: one is copied to the other
ds_site, dbh_site = DeviceMatrix.zeros(B, N1, dev), torch.zeros(N1, dtype=torch.float32, device=dev)
hv_out = DeviceMatrix.zeros(B, N1, dev)
ws_top, ws_aux = top.disc_workspace(B, C), aux1.disc_workspace(B, C)
LR = 0.0                     # the launches and their traffic are those of a training step, the parameters stay where they are


def forward():
    l1.probs_into(V, B, 0, ACT_SIGMOID, x1)
    l2.probs_into(x1, B, 0, ACT_SIGMOID, plane)
    plane.t[:B, N2:N2 + C].copy_(onehot)


def top_back():
    return top.disc_backprop(plane, C, B, 0, e_in=e2, ws=ws_top)[0]


def back2():
    return l2.backprop_layer(ACT_SIGMOID, x1, plane, e2, B, 0, e_in=e1)


def back1():
    return l1.backprop_layer(ACT_SIGMOID, V, x1, e1, B, 0)


def applies(d1=None, d2=None, dt=None):
    l1.apply_delta(LR, which=3, delta=d1)
    l2.apply_delta(LR, which=3, delta=d2)
    top.apply_delta(LR, delta=dt)


def step():
    forward()
    dt = top_back()
    d2 = back2()
    d1 = back1()
    applies(d1, d2, dt)


def site():
    # (the C call on planes made once: the engine's method allocates its outputs per call)
    check(l1.lib.kurbm_backprop_delta(l1.ctx.handle, es_site.ptr(), es_site.ld, xs_site.ptr(), xs_site.ld, B, N1, ACT_SIGMOID, ds_site.ptr(),
                                      ds_site.ld, dbh_site.data_ptr(), ws_site.data_ptr(), ws_site.numel(), l1._stream()))


def copy():
    n = half.numel() // 2
    half[n:].copy_(half[:n])


def stage3(eng, v, ws):
    eng.ctx.set_option("KURBM_DISC_STAGE", 3)
    eng.class_grad(v, C, want_planes=False, want_nll=False, ws=ws)
    eng.ctx.set_option("KURBM_DISC_STAGE", 0)


def linear_hv():
    check(l2.lib.kurbm_half_step_hv(l2.ctx.handle, C_.byref(l2.params), e2.ptr(), B, e2.ld, ACT_LINEAR, NOISE_NONE, None, None, hv_out.ptr(),
                                    hv_out.ld, l2._stream()))


variants = {
    "fine-tune step (all of the below)": step,
    "forward: two half steps, one-hot block": forward,
    "top: kurbm_disc_backprop": top_back,
    "layer 2: kurbm_backprop_layer": back2,
    "layer 1: kurbm_backprop_layer (no e_in)": back1,
    "applies: three kurbm_apply_delta": applies,
    "(a) k_backprop_delta + k_backprop_reduce": site,
    "(a) device-to-device copy, same bytes": copy,
    "(b) top: kurbm_class_grad": lambda: top.class_grad(plane, C, want_planes=False, want_nll=False, ws=ws_top),
    "(b) v -> h half step, layer 1": lambda: l1.probs_into(V, B, 0, ACT_SIGMOID, x1),
    "(b) v -> h half step, layer 2": lambda: l2.probs_into(x1, B, 0, ACT_SIGMOID, plane),
    "(b) linear h -> v half step, layer 2": linear_hv,
    "(b) statistics GEMM + reductions, layer 1": lambda: stage3(aux1, VL, ws_aux),
    "(b) statistics GEMM + reductions, layer 2": lambda: stage3(top, plane, ws_top),
}


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


step()                                                                   # complete calls: the planes the staged calls run on
aux1.class_grad(VL, C, want_planes=False, want_nll=False, ws=ws_aux)
for fn in variants.values():          # the common warm-up: code objects loaded, workspaces allocated
    window(fn, 5)
times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, fn in variants.items():
        times[name].append(window(fn, args.calls))
med = {name: statistics.median(ts) for name, ts in times.items()}
names = list(variants)
plane_mb = B * N1 * 4 / 1e6
lines = ["fine-tuning a DBN, %d -> %d -> %d under %d + %d -> %d, batch %d, fp32 path; %s" % (N0, N1, N2, N2, C, NT, B, torch.cuda.get_device_name(0)),
         "us per call: device events around %d queued calls, median of %d windows (all windows listed), variants alternating" % (args.calls, args.rounds)]
for name in names:
    lines.append("%-42s %8.1f us   (%s)" % (name, med[name], " ".join("%.1f" % x for x in times[name])))
t_site, t_copy = med[names[6]], med[names[7]]
lines.append("(a) the site: three planes of %d x %d floats = %.1f MB in %.1f us = %.2f TB/s; the copy moves them in %.1f us = %.2f TB/s; ratio %.2f x"
             % (B, N1, 3 * plane_mb, t_site, 3 * plane_mb / t_site, t_copy, 3 * plane_mb / t_copy, t_site / t_copy))
parts = sum(med[n] for n in names[1:6])
existing = sum(med[n] for n in names[8:]) + med[names[5]]
spread = max(max(ts) - min(ts) for n, ts in times.items() if n in names[8:] or n == names[5] or n == names[6])
lines.append("the step against the sum of its launch groups: %.1f us against %.1f us (%+.1f us)" % (med[names[0]], parts, med[names[0]] - parts))
lines.append("(b) the step against the existing calls it is made of + (a) per lower layer: %.1f us against %.1f + 2 x %.1f = %.1f us (%+.1f us = %+.1f %%;"
             % (med[names[0]], existing, t_site, existing + 2 * t_site, med[names[0]] - existing - 2 * t_site,
                100.0 * (med[names[0]] / (existing + 2 * t_site) - 1.0)))
lines.append("  the largest run-to-run spread of one of those terms' windows: %.1f us)" % spread)
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
