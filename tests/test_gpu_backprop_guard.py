"""GPU tier: the entry points of DBN fine-tuning -- kurbm_backprop_delta, kurbm_backprop_layer, kurbm_disc_backprop -- on a guarded
arena (tests/guarded.py): every buffer exactly its size query between two guards, every plane and W with wide leading dimensions
(ld % 8 == 4) and NaN padding, the workspace NaN-filled, the padding of every output poisoned.  Guards, padding and inputs must
come back untouched, the results bit for bit those of the same call on ordinary buffers, and a workspace 16 bytes short must be
refused with nothing changed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # guarded.py and the restatements live beside this file
import backprop_ref as B
import labels_ref as R
from guarded import Arena, GuardedRBM

pytestmark = pytest.mark.gpu

ROWS, NIN, NOUT, NC, NTOP = 70, 37, 53, 10, 20       # a layer NIN -> NOUT (n_hid % 4 == 1) under a NOUT + NC -> NTOP top
KURBM_ERR_WORKSPACE = -4


def eq(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: the guarded run differs from the plain run" % what


def _dm(x, dev):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    return DeviceMatrix.from_host(np.array(x, dtype=np.float32), dev)


def _layer_problem(act):
    g = np.random.default_rng(5400 + act)
    W = g.normal(0, .1, (NIN, NOUT)).astype(np.float32)
    b_h = g.normal(0, .3, NOUT).astype(np.float32)
    x_in = (g.random((ROWS, NIN)) < .5).astype(np.float32)
    x_out = B.activate(x_in.astype(np.float64) @ W + b_h, act).astype(np.float32)
    e = g.normal(0, 1, (ROWS, NOUT)).astype(np.float32)
    return W, b_h, np.zeros(NIN, np.float32), x_in, x_out, e


def _pair(dev, W, b_h, b_v):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    arena = Arena(dev, capacity=96 << 20)
    return DeviceRBM(W, b_h, b_v, dev), GuardedRBM(arena, W, b_h, b_v, dev), arena


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU, B.ACT_LINEAR], ids=["sigmoid", "relu", "linear"])
def test_site_guarded(gpu_device, act, in_place):
    W, b_h, b_v, _, x_out, e = _layer_problem(act)
    A, G, arena = _pair(gpu_device, W, b_h, b_v)
    G.freeze_params()
    xg = arena.carve_matrix(ROWS, NOUT, data=x_out, name="x_out")                     # wide ld, NaN padding, frozen
    eg = arena.carve_matrix(ROWS, NOUT, data=e, name="e", kind="inout" if in_place else "input")
    da, ha = A.backprop_delta(_dm(e, gpu_device), _dm(x_out, gpu_device), act, in_place=in_place)
    dg, hg = G.backprop_delta(eg, xg, act, in_place=in_place)                         # its workspace: exactly the query, NaN-filled
    arena.check()
    assert xg.ld % 8 == 4 and dg.ld > da.ld, "the guarded planes have wide leading dimensions"
    eq(da.view(), dg.view(), "delta")
    eq(ha, hg, "db_h")
    assert bool(torch.isfinite(dg.view()).all().item()) and bool(torch.isfinite(hg).all().item())


@pytest.mark.parametrize("with_e_in", [True, False], ids=["e_in", "no-e_in"])
@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
def test_layer_guarded(gpu_device, act, with_e_in):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    W, b_h, b_v, x_in, x_out, e = _layer_problem(act)
    A, G, arena = _pair(gpu_device, W, b_h, b_v)
    G.freeze_params()
    xi = arena.carve_matrix(ROWS, NIN, data=x_in, name="x_in")
    xo = arena.carve_matrix(ROWS, NOUT, data=x_out, name="x_out")
    eg = arena.carve_matrix(ROWS, NOUT, data=e, name="e", kind="inout")
    ei_g = arena.carve_matrix(ROWS, NIN, name="e_in") if with_e_in else None           # an output: poisoned padding
    ei_a = DeviceMatrix.zeros(ROWS, NIN, gpu_device) if with_e_in else None
    ea = _dm(e, gpu_device)
    da = A.backprop_layer(act, _dm(x_in, gpu_device), _dm(x_out, gpu_device), ea, e_in=ei_a)
    dg = G.backprop_layer(act, xi, xo, eg, e_in=ei_g)                                  # workspace and delta: exact carves, NaN-filled
    arena.check()
    assert xi.ld % 8 == 4 and G.W.ld % 8 == 4
    eq(da, dg, "delta_out")
    eq(ea.view(), eg.view(), "delta (in place over e)")
    assert bool(torch.isfinite(dg).all().item())
    if with_e_in:
        eq(ei_a.view(), ei_g.view(), "e_in")
        assert bool(torch.isfinite(ei_g.view()).all().item())


@pytest.mark.parametrize("with_e_in", [True, False], ids=["e_in", "no-e_in"])
def test_disc_backprop_guarded(gpu_device, with_e_in):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    W, b_h, b_v = R.model(NOUT, NC, NTOP, std=.1)
    V, _ = R.labelled_batch(ROWS, NOUT, NC)
    A, G, arena = _pair(gpu_device, W, b_h, b_v)
    G.freeze_params()
    vg = arena.carve_matrix(ROWS, NOUT + NC, data=V, name="v_batch")
    ei_g = arena.carve_matrix(ROWS, NOUT, name="e_in") if with_e_in else None
    ei_a = DeviceMatrix.zeros(ROWS, NOUT, gpu_device) if with_e_in else None
    da, na = A.disc_backprop(_dm(V, gpu_device), NC, e_in=ei_a, want_nll=True)
    need = int(G.lib.kurbm_disc_workspace_bytes(G.ctx.handle, ROWS, NOUT + NC, NTOP, NC))
    ws = arena.carve(need, "disc_ws")                                                  # exactly the query (no ldv addition), NaN-filled
    dg, ng = G.disc_backprop(vg, NC, e_in=ei_g, want_nll=True, ws=ws)
    arena.check()
    eq(da, dg, "delta_out")
    eq(na, ng, "nll_mean")
    assert bool(torch.isfinite(dg).all().item()) and bool(torch.isfinite(ng).all().item())
    if with_e_in:
        eq(ei_a.view(), ei_g.view(), "e_in")
        assert bool(torch.isfinite(ei_g.view()).all().item())


def test_short_workspace_refused(gpu_device):
    W, b_h, b_v, x_in, x_out, e = _layer_problem(B.ACT_SIGMOID)
    _, G, arena = _pair(gpu_device, W, b_h, b_v)
    Wt, bht, bvt = R.model(NOUT, NC, NTOP, std=.1)
    T = GuardedRBM(arena, Wt, bht, bvt, gpu_device)
    V, _ = R.labelled_batch(ROWS, NOUT, NC)
    lib, ctx = G.lib, G.ctx.handle
    xi = arena.carve_matrix(ROWS, NIN, data=x_in, name="x_in")
    xo = arena.carve_matrix(ROWS, NOUT, data=x_out, name="x_out")
    eg = arena.carve_matrix(ROWS, NOUT, data=e, name="e", kind="inout")
    ei = arena.carve_matrix(ROWS, NIN, name="e_in")
    dd = arena.carve_matrix(ROWS, NOUT, name="delta")
    vg = arena.carve_matrix(ROWS, NOUT + NC, data=V, name="v_batch")
    et = arena.carve_matrix(ROWS, NOUT, name="e_top")
    need = int(lib.kurbm_backprop_workspace_bytes(ctx, ROWS, NIN, NOUT))
    need1 = int(lib.kurbm_backprop_workspace_bytes(ctx, ROWS, 1, NOUT))
    needt = int(lib.kurbm_disc_workspace_bytes(ctx, ROWS, NOUT + NC, NTOP, NC))
    assert min(need, need1, needt) > 16
    ws, short = arena.carve(need, "ws"), arena.carve(need - 16, "short_ws")
    ws1, short1 = arena.carve(need1, "site_ws"), arena.carve(need1 - 16, "short_site_ws")
    wst, shortt = arena.carve(needt, "top_ws"), arena.carve(needt - 16, "short_top_ws")
    delta = arena.carve_floats(NIN * NOUT + NOUT + NIN, "delta_out")
    tdelta = arena.carve_floats((NOUT + NC) * NTOP + NTOP + NOUT + NC, "top_delta_out")
    db_h = arena.carve_floats(NOUT, "db_h")
    arena.freeze_all()
    P, TP, st = C.byref(G.params), C.byref(T.params), G._stream()

    def site(w):
        return lib.kurbm_backprop_delta(ctx, eg.ptr(), eg.ld, xo.ptr(), xo.ld, ROWS, NOUT, B.ACT_SIGMOID, dd.ptr(), dd.ld, db_h.data_ptr(),
                                        w.data_ptr(), w.numel(), st)

    def layer(w):
        return lib.kurbm_backprop_layer(ctx, P, B.ACT_SIGMOID, xi.ptr(), xi.ld, xo.ptr(), xo.ld, eg.ptr(), eg.ld, ROWS, delta.data_ptr(),
                                        ei.ptr(), ei.ld, w.data_ptr(), w.numel(), st)

    def disc(w):
        return lib.kurbm_disc_backprop(ctx, TP, NC, vg.ptr(), ROWS, vg.ld, tdelta.data_ptr(), et.ptr(), et.ld, None, w.data_ptr(), w.numel(), st)

    for call in (lambda: site(short1), lambda: layer(short), lambda: disc(shortt)):
        assert call() == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    arena.check()
    # ... and the same calls with the full sizes are accepted
    for b in arena.bufs:
        b.frozen = None
    assert site(ws1) == 0 and layer(ws) == 0 and disc(wst) == 0
    arena.check()
