"""GPU tier: the three new entry points of the softmax label units -- kurbm_label_sample, kurbm_cd_step_labels (and the epoch
call), kurbm_class_logits -- on a guarded arena (tests/guarded.py): every buffer exactly its size query between two guards, h / v
/ W with wide leading dimensions and NaN padding, the workspace NaN-filled, the padding of every output poisoned.  Guards, padding
and inputs must come back untouched, the results bit for bit those of the same call on ordinary buffers, and a workspace 16 bytes
short must be refused with nothing changed."""
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
LR, SEED, STEP = 1e-3, 42, 3


def eq(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: the guarded run differs from the plain run" % what


@pytest.fixture()
def pair(gpu_device):
    """(plain DeviceRBM, GuardedRBM, arena, the parameters)."""
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    W, b_h, b_v = R.model(NPIX, NC, NH)
    arena = Arena(gpu_device, capacity=64 << 20)
    return DeviceRBM(W, b_h, b_v, gpu_device), GuardedRBM(arena, W, b_h, b_v, gpu_device), arena, (W, b_h, b_v)


def _dm(x, dev):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    return DeviceMatrix.from_host(np.ascontiguousarray(x, dtype=np.float32), dev)


# (n_hid, classes): the guarded tail of the kernel alone; three and four full 64-unit blocks -- the unconditional loads of its
# main loop next to the NaN padding of h and W -- with one and with four blocks of classes
@pytest.mark.parametrize("NH,NC", [(52, 10), (200, 10), (260, 40)])
def test_label_sample_guarded(gpu_device, NH, NC):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    NV = NPIX + NC
    W, b_h, b_v = R.model(NPIX, NC, NH)
    arena = Arena(gpu_device, capacity=64 << 20)
    A, B = DeviceRBM(W, b_h, b_v, gpu_device), GuardedRBM(arena, W, b_h, b_v, gpu_device)
    B.freeze_params()
    h = (np.random.default_rng(3).random((ROWS, NH)) < .5).astype(np.float32)
    v0 = np.random.default_rng(8).normal(0, 1, (ROWS, NV)).astype(np.float32)
    hb = arena.carve_matrix(ROWS, NH, data=h, name="h")                              # wide ld, NaN padding, frozen
    vb = arena.carve_matrix(ROWS, NV, data=v0, name="v", kind="inout")               # its padding must not change
    va = _dm(v0, gpu_device)
    oa = A.label_sample(_dm(h, gpu_device), va, NC, SEED, 1, 7, want_prob=True, want_u=True)
    ob = B.label_sample(hb, vb, NC, SEED, 1, 7, want_prob=True, want_u=True)
    arena.check()
    assert vb.ld > va.ld and ob["prob"].ld > oa["prob"].ld, "the guarded buffers have wide leading dimensions"
    eq(va.view(), vb.view(), "v")
    eq(oa["prob"].view(), ob["prob"].view(), "prob")
    eq(oa["u"], ob["u"], "u")
    got = vb.to_numpy()
    assert np.array_equal(got[:, :NPIX].view(np.uint32), v0[:, :NPIX].view(np.uint32)), "pixel columns were written"
    assert np.array_equal(got[:, NPIX:].sum(axis=1), np.ones(ROWS)) and bool(torch.isfinite(ob["prob"].view()).all().item())
    # ... and the plain run is the restatement's: every row's class, the probabilities at the project's bound
    p_ref, _, cls_ref, margin = R.label_site(W, b_v, h, NPIX, SEED, 1, 7)
    assert float(np.max(np.abs(ob["prob"].to_numpy() - p_ref))) <= R.TOL_P
    assert margin.min() > 5e-4, "fixture: a draw close to a cumulative boundary"       # (8e-4 at least for these inputs)
    assert np.array_equal(got[:, NPIX:].argmax(axis=1), cls_ref)


@pytest.mark.parametrize("variant", ["apply", "emit", "k2-chain", "mom", "epoch"])
def test_cd_step_labels_guarded(gpu_device, pair, variant):
    A, B, arena, params = pair
    n = 150 if variant == "epoch" else ROWS
    V, _ = R.labelled_batch(n, NPIX, NC)
    va, vb = _dm(V, gpu_device), arena.carve_matrix(n, NV, data=V, name="v_batch")
    ca = cb = None
    kw = dict(n_labels=NC)
    if variant == "emit":
        kw.update(apply=False, emit_delta=True)
        B.freeze_params()
    if variant == "k2-chain":
        chain0, _ = R.labelled_batch(ROWS, NPIX, NC, seed=6)
        ca, cb = _dm(chain0, gpu_device), arena.carve_matrix(ROWS, NV, data=chain0, name="v_chain", kind="inout")
        assert cb.ld == vb.ld
        kw.update(k=2, v_chain=ca)
    if variant == "mom":
        kw.update(momentum=(0.9, 1e-3), emit_delta=True)
    if variant == "epoch":
        assert A.cd_epoch(va, n, 64, LR, SEED, STEP, **kw) == 3 and B.cd_epoch(vb, n, 64, LR, SEED, STEP, **kw) == 3
    else:
        A.cd_step(va, ROWS, 0, LR, SEED, STEP, **kw)
        if ca is not None:
            kw.update(v_chain=cb)
        B.cd_step(vb, ROWS, 0, LR, SEED, STEP, **kw)
    arena.check()
    A.check_status()
    for x, y, name in zip(A.get_weights(), B.get_weights(), ("W", "b_h", "b_v")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    if kw.get("emit_delta"):
        eq(A.delta, B.delta, "delta")
        assert bool(torch.isfinite(B.delta).all().item())
    if variant == "mom":
        eq(A.velocity, B.velocity, "velocity")
    if variant == "emit":
        assert np.array_equal(B.get_weights()[0], params[0])
    else:
        assert np.isfinite(B.get_weights()[0]).all() and not np.array_equal(B.get_weights()[0], params[0])
    if ca is not None:
        eq(ca.view(), cb.view(), "v_chain")
        assert np.array_equal(cb.to_numpy()[:, NPIX:].sum(axis=1), np.ones(ROWS))


@pytest.mark.parametrize("wide", [False, True], ids=["pixels", "pixels+block"])
def test_class_logits_guarded(gpu_device, pair, wide):
    A, B, arena, _ = pair
    B.freeze_params()
    v = np.random.default_rng(6).normal(0, 1, (ROWS, NV if wide else NPIX)).astype(np.float32)
    vb = arena.carve_matrix(ROWS, v.shape[1], data=v, name="v")
    la, pa = A.class_logits(_dm(v, gpu_device), NC)
    lb, pb = B.class_logits(vb, NC)
    arena.check()
    assert lb.ld > la.ld
    eq(la.view(), lb.view(), "logits")
    eq(pa.view(), pb.view(), "prob")
    assert bool(torch.isfinite(lb.view()).all().item()) and bool(torch.isfinite(pb.view()).all().item())


def test_short_workspace_refused(gpu_device, pair):
    from keras_unsupervised_amd._lib import CdOpts
    _, B, arena, _ = pair
    lib, ctx = B.lib, B.ctx.handle
    V, _ = R.labelled_batch(ROWS, NPIX, NC)
    vb = arena.carve_matrix(ROWS, NV, data=V, name="v_batch")
    need = int(lib.kurbm_workspace_bytes(ctx, ROWS, NV, NH, 1))
    need += -(-ROWS * vb.ld * 4 // 256) * 256 - (-(-ROWS * 48 * 4 // 256) * 256)      # the ldv addition of include/kurbm.h
    cneed = int(lib.kurbm_class_workspace_bytes(ctx, ROWS, NV, NH))
    assert need > 16 and cneed > 16
    ws, short_ws = arena.carve(need, "ws"), arena.carve(need - 16, "short_ws")
    cws, short_cws = arena.carve(cneed, "class_ws"), arena.carve(cneed - 16, "short_class_ws")
    delta = arena.carve_floats(NV * NH + NH + NV, "delta")
    logits, prob = arena.carve_matrix(ROWS, NC, name="logits"), arena.carve_matrix(ROWS, NC, name="prob")
    assert logits.ld == prob.ld
    arena.freeze_all()
    opts = CdOpts(1, 0, LR, 1, delta.data_ptr(), None, SEED, 0, STEP, 0)

    def step(w):
        return lib.kurbm_cd_step_labels(ctx, C.byref(B.params), NC, vb.ptr(), ROWS, vb.ld, C.byref(opts), 7, w.data_ptr(), w.numel(),
                                        B._stream(), None)

    def epoch(w):
        o = CdOpts(1, 0, LR, 1, None, None, SEED, 0, STEP, 0)
        return lib.kurbm_cd_epoch_labels(ctx, C.byref(B.params), NC, vb.ptr(), ROWS, vb.ld, ROWS, C.byref(o), w.data_ptr(), w.numel(),
                                         B._stream(), None)

    def logit(w):
        return lib.kurbm_class_logits(ctx, C.byref(B.params), NC, vb.ptr(), ROWS, vb.ld, logits.ptr(), logits.ld, prob.ptr(),
                                      w.data_ptr(), w.numel(), B._stream())

    for call, w in ((step, short_ws), (epoch, short_ws), (logit, short_cws)):
        assert call(w) == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    arena.check()
    # ... and the same calls with the full sizes are accepted
    for b in arena.bufs:
        b.frozen = None
    assert logit(cws) == 0 and step(ws) == 0
    arena.check()
