"""GPU tier: kurbm_gibbs_run on a guarded arena (tests/guarded.py) -- every buffer exactly its size query between two guards,
v_init and W with wide leading dimensions and NaN padding, the workspace and the mirror NaN-filled, the padding of v_out /
prob_out poisoned.  Guards, padding and inputs must come back untouched, the results bit for bit those of the same call on
ordinary buffers, and a workspace or mirror 16 bytes short must be refused with nothing changed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # guarded.py and gibbs_ref.py live beside this file
import gibbs_ref as R
from guarded import Arena, GuardedRBM

pytestmark = pytest.mark.gpu

ROWS, NV, NH = 37, 70, 36
KURBM_ERR_WORKSPACE = -4


def eq(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: the guarded run differs from the plain run" % what


@pytest.fixture()
def pair(gpu_device):
    """(plain DeviceRBM, GuardedRBM with frozen parameters, arena)."""
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    W, b_h, b_v = R.normal_params(31, NV, NH, 0.3, 0.3)
    arena = Arena(gpu_device, capacity=64 << 20)
    A, B = DeviceRBM(W, b_h, b_v, gpu_device), GuardedRBM(arena, W, b_h, b_v, gpu_device)
    B.freeze_params()
    return A, B, arena


def start(mode, real):
    g = np.random.default_rng(3)
    if mode == R.MODE_GAUSSIAN:
        return g.normal(0.0, 1.0, (ROWS, NV)).astype(np.float32)
    v = (g.random((ROWS, NV)) < 0.5).astype(np.float32)
    if real:
        v[:, R.CLAMP_COLS] = g.random((ROWS, R.CLAMP_COLS.size)).astype(np.float32)
    return v


@pytest.mark.parametrize("mode,clamped,real", [(R.MODE_BERNOULLI, False, False), (R.MODE_BERNOULLI, True, False),
                                               (R.MODE_BERNOULLI, True, True), (R.MODE_GAUSSIAN, False, False),
                                               (R.MODE_GAUSSIAN, True, False)])
def test_gibbs_run_guarded(gpu_device, pair, mode, clamped, real):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    A, B, arena = pair
    v = start(mode, real)
    mask = np.zeros(NV, dtype=bool)
    mask[R.CLAMP_COLS] = True
    vb = arena.carve_matrix(ROWS, NV, data=v, name="v_init")          # wide ld, NaN padding, frozen
    cb = None
    if clamped:
        cb = arena.carve(NV, "clamp")
        cb.copy_(torch.from_numpy(mask.astype(np.uint8)))
        arena.freeze(cb)
    kw = dict(burn_in=2, thin=2, n_keep=2, chain0=8, seed=9, mode=mode, want_prob=True)
    va, pa = A.gibbs_run(DeviceMatrix.from_host(v, gpu_device), clamp=mask if clamped else None, **kw)
    vg, pg = B.gibbs_run(vb, clamp=cb, **kw)
    arena.check()
    A.check_status()
    assert vg.ld > va.ld and pg.ld > pa.ld, "the guarded outputs have wide leading dimensions"
    eq(va.view(), vg.view(), "v_out")
    eq(pa.view(), pg.view(), "prob_out")
    assert bool(torch.isfinite(vg.view()).all().item()) and bool(torch.isfinite(pg.view()).all().item())
    if clamped:
        want = torch.from_numpy(v[:, R.CLAMP_COLS]).to(gpu_device)
        for j in range(2):
            eq(vg.view()[j * ROWS:(j + 1) * ROWS][:, R.CLAMP_COLS.tolist()], want, "clamped columns of kept plane %d" % j)


@pytest.mark.parametrize("mode", [R.MODE_BERNOULLI, R.MODE_GAUSSIAN])
def test_short_workspace_and_mirror_refused(gpu_device, pair, mode):
    from keras_unsupervised_amd import _lib
    _, B, arena = pair
    lib, ctx = B.lib, B.ctx.handle
    vp = (1 | _lib.V_BINARY) if mode == R.MODE_BERNOULLI else 3
    need = int(lib.kurbm_gibbs_workspace_bytes(ctx, ROWS, NV, NH, vp, mode))
    mneed = int(lib.kurbm_x3_mirror_bytes(ctx, NV, NH))
    assert need > 16 and mneed > 16
    ws, short_ws = arena.carve(need, "ws"), arena.carve(need - 16, "short_ws")
    mir, short_mir = arena.carve(mneed, "mirror"), arena.carve(mneed - 16, "short_mirror")
    vb = arena.carve_matrix(ROWS, NV, data=start(mode, False), name="v_init")
    vo, po = arena.carve_matrix(ROWS, NV, name="v_out"), arena.carve_matrix(ROWS, NV, name="prob_out")
    cb = arena.carve(NV, "clamp")
    cb.zero_()
    arena.freeze_all()

    def call(m, w):
        return lib.kurbm_gibbs_run(ctx, C.byref(B.params), m.data_ptr(), m.numel(), vb.ptr(), vp, vb.ld, ROWS, 0, 9, mode, 2, 1, 1,
                                   cb.data_ptr(), vo.ptr(), po.ptr(), vo.ld, 0, w.data_ptr(), w.numel(), B._stream())

    assert call(mir, short_ws) == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    assert call(short_mir, ws) == KURBM_ERR_WORKSPACE and b"mirror too small" in lib.kurbm_last_error()
    arena.check()
