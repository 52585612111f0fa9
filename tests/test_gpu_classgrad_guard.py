"""GPU tier: the entry points of discriminative / hybrid training -- kurbm_class_grad, kurbm_disc_step, kurbm_disc_epoch -- on a
guarded arena (tests/guarded.py): every buffer exactly its size query between two guards, the batch, the persistent chain and W
with wide leading dimensions (ld % 8 == 4) and NaN padding, the workspace NaN-filled, the padding of every output poisoned.
Guards, padding and inputs must come back untouched, the results bit for bit those of the same call on ordinary buffers, and a
workspace 16 bytes short must be refused with nothing changed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # guarded.py and labels_ref.py live beside this file
import labels_ref as R
from guarded import Arena, GuardedRBM

pytestmark = pytest.mark.gpu

ROWS, NPIX, NC, NH = 70, 37, 10, 52
NV = NPIX + NC
KURBM_ERR_WORKSPACE = -4
LR, SEED, STEP, GW = 1e-3, 42, 3, 0.01


def eq(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: the guarded run differs from the plain run" % what


def _dm(x, dev):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    return DeviceMatrix.from_host(np.ascontiguousarray(x, dtype=np.float32), dev)


def _pair(dev, n_pix=NPIX, C_=NC, n_hid=NH):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    W, b_h, b_v = R.model(n_pix, C_, n_hid)
    arena = Arena(dev, capacity=64 << 20)
    return DeviceRBM(W, b_h, b_v, dev), GuardedRBM(arena, W, b_h, b_v, dev), arena, (W, b_h, b_v)


def _hybrid_need(B, rows, ldv, n_vis=NV, n_hid=NH, C_=NC):
    """kurbm_disc_workspace_bytes plus the ldv addition of include/kurbm.h (a hybrid step on a wide batch)."""
    need = int(B.lib.kurbm_disc_workspace_bytes(B.ctx.handle, rows, n_vis, n_hid, C_))
    ldc = -(-n_vis // 4) * 4
    return need + -(-rows * ldv * 4 // 256) * 256 - (-(-rows * ldc * 4 // 256) * 256)


# (n_pix, classes, n_hid): the label fixtures' shape; the C > 16 template with n_hid % 4 == 1 -- a column tail next to the NaN
# padding of the planes and of W
@pytest.mark.parametrize("n_pix,C_,n_hid", [(NPIX, NC, NH), (33, 17, 129)])
def test_class_grad_guarded(gpu_device, n_pix, C_, n_hid):
    A, B, arena, params = _pair(gpu_device, n_pix, C_, n_hid)
    B.freeze_params()
    V, _ = R.labelled_batch(ROWS, n_pix, C_)
    vb = arena.carve_matrix(ROWS, n_pix + C_, data=V, name="v_batch")                 # wide ld, NaN padding, frozen
    oa = A.class_grad(_dm(V, gpu_device), C_)
    ob = B.class_grad(vb, C_)                                                         # its workspace: exactly the query, NaN-filled
    arena.check()
    assert vb.ld % 8 == 4 and B.W.ld % 8 == 4 and ob["S_y"].ld > oa["S_y"].ld, "the guarded buffers have wide leading dimensions"
    for k in ("S_y", "H_bar"):
        eq(oa[k].view(), ob[k].view(), k)
    eq(oa["nll"], ob["nll"], "nll")
    eq(oa["delta"], ob["delta"], "delta")
    assert bool(torch.isfinite(ob["delta"]).all().item()) and bool(torch.isfinite(ob["S_y"].view()).all().item())
    assert bool(torch.isfinite(ob["nll"]).all().item())
    # the hook without its optional outputs
    ob2 = B.class_grad(vb, C_, want_planes=False, want_nll=False)
    arena.check()
    eq(oa["delta"], ob2["delta"], "delta (no planes)")


@pytest.mark.parametrize("variant", ["disc", "disc-mom", "hybrid", "hybrid-k2-chain", "hybrid-mom"])
def test_disc_step_guarded(gpu_device, variant):
    A, B, arena, params = _pair(gpu_device)
    V, _ = R.labelled_batch(ROWS, NPIX, NC)
    va, vb = _dm(V, gpu_device), arena.carve_matrix(ROWS, NV, data=V, name="v_batch")
    hybrid = variant.startswith("hybrid")
    kw = dict(gen_weight=GW if hybrid else 0.0, seed=SEED, step=STEP, want_nll=True)
    ca = cb = None
    if variant.endswith("mom"):
        kw.update(momentum=(0.9, 1e-3))
    if variant == "hybrid-k2-chain":
        chain0, _ = R.labelled_batch(ROWS, NPIX, NC, seed=6)
        ca, cb = _dm(chain0, gpu_device), arena.carve_matrix(ROWS, NV, data=chain0, name="v_chain", kind="inout")
        assert cb.ld == vb.ld
        kw.update(k=2)
    need = _hybrid_need(B, ROWS, vb.ld) if hybrid else int(B.lib.kurbm_disc_workspace_bytes(B.ctx.handle, ROWS, NV, NH, NC))
    ws = arena.carve(need, "disc_ws")                                                  # exactly what the header says, NaN-filled
    na = A.disc_step(va, ROWS, 0, LR, NC, v_chain=ca, **kw)
    nb = B.disc_step(vb, ROWS, 0, LR, NC, v_chain=cb, ws=ws, **kw)
    arena.check()
    A.check_status()
    for x, y, name in zip(A.get_weights(), B.get_weights(), ("W", "b_h", "b_v")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    eq(na, nb, "nll_mean")
    assert np.isfinite(B.get_weights()[0]).all() and not np.array_equal(B.get_weights()[0], params[0]) and bool(torch.isfinite(nb).all().item())
    if "momentum" in kw:
        eq(A.velocity, B.velocity, "velocity")
    if ca is not None:
        eq(ca.view(), cb.view(), "v_chain")
        assert np.array_equal(cb.to_numpy()[:, NPIX:].sum(axis=1), np.ones(ROWS))


@pytest.mark.parametrize("gw", [0.0, GW], ids=["disc", "hybrid"])
def test_disc_epoch_guarded(gpu_device, gw):
    A, B, arena, params = _pair(gpu_device)
    n = 150
    V, _ = R.labelled_batch(n, NPIX, NC)
    va, vb = _dm(V, gpu_device), arena.carve_matrix(n, NV, data=V, name="V")
    need = _hybrid_need(B, 64, vb.ld) if gw else int(B.lib.kurbm_disc_workspace_bytes(B.ctx.handle, 64, NV, NH, NC))
    ws = arena.carve(need, "disc_ws")
    sa, na = A.disc_epoch(va, n, 64, LR, NC, gen_weight=gw, seed=SEED, step0=STEP, want_nll=True)
    sb, nb = B.disc_epoch(vb, n, 64, LR, NC, gen_weight=gw, seed=SEED, step0=STEP, want_nll=True, ws=ws)
    arena.check()
    assert sa == sb == 3
    for x, y, name in zip(A.get_weights(), B.get_weights(), ("W", "b_h", "b_v")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    eq(na[:3], nb[:3], "nll_means")
    assert np.isfinite(B.get_weights()[0]).all() and not np.array_equal(B.get_weights()[0], params[0])


def test_short_workspace_refused(gpu_device):
    from keras_unsupervised_amd._lib import CdOpts
    _, B, arena, _ = _pair(gpu_device)
    lib, ctx = B.lib, B.ctx.handle
    V, _ = R.labelled_batch(ROWS, NPIX, NC)
    vb = arena.carve_matrix(ROWS, NV, data=V, name="v_batch")
    need = int(lib.kurbm_disc_workspace_bytes(ctx, ROWS, NV, NH, NC))
    hneed = _hybrid_need(B, ROWS, vb.ld)
    assert hneed > need > 16
    ws, short_ws = arena.carve(need, "ws"), arena.carve(need - 16, "short_ws")
    hws, short_hws = arena.carve(hneed, "hybrid_ws"), arena.carve(hneed - 16, "short_hybrid_ws")
    delta = arena.carve_floats(NV * NH + NH + NV, "delta")
    nll_mean = arena.carve_floats(4, "nll_mean")
    arena.freeze_all()
    opts = CdOpts(1, 0, LR, 1, None, None, SEED, 0, STEP, 0)
    P, O, st = C.byref(B.params), C.byref(opts), B._stream()

    def hook(w):
        return lib.kurbm_class_grad(ctx, P, NC, vb.ptr(), ROWS, vb.ld, None, None, 0, None, delta.data_ptr(), w.data_ptr(), w.numel(), st)

    def step(w, gw=0.0):
        return lib.kurbm_disc_step(ctx, P, NC, vb.ptr(), ROWS, vb.ld, O, gw, nll_mean.data_ptr(), w.data_ptr(), w.numel(), st, None)

    def epoch(w, gw=0.0):
        return lib.kurbm_disc_epoch(ctx, P, NC, vb.ptr(), ROWS, vb.ld, ROWS, O, gw, nll_mean.data_ptr(), w.data_ptr(), w.numel(), st, None)

    for call in (lambda: hook(short_ws), lambda: step(short_ws), lambda: epoch(short_ws), lambda: step(short_hws, GW),
                 lambda: epoch(short_hws, GW), lambda: step(ws, GW)):      # (the last: a hybrid step needs the ldv addition)
        assert call() == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    arena.check()
    # ... and the same calls with the full sizes are accepted
    for b in arena.bufs:
        b.frozen = None
    assert hook(ws) == 0 and step(ws) == 0 and step(hws, GW) == 0 and epoch(hws, GW) == 1
    arena.check()
