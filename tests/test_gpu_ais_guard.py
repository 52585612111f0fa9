"""GPU tier: kurbm_ais_step and kurbm_ais_run on a guarded arena (tests/guarded.py) -- every buffer exactly its size query
between two guards, matrices with wide leading dimensions, the workspace NaN-filled, output padding poisoned.  Guards, padding
and inputs must come back untouched, the results bit for bit those of the same call on ordinary buffers, and a workspace 16 bytes
short must be refused with nothing changed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # guarded.py and ais_ref.py live beside this file
import ais_ref as R
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
    """(plain DeviceRBM, GuardedRBM with frozen parameters, arena, b_A host, b_A carved and frozen, v host)."""
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    W, b_h, b_v, b_a = R.normal_params(31, NV, NH, 0.3, 0.3)
    arena = Arena(gpu_device, capacity=64 << 20)
    A, B = DeviceRBM(W, b_h, b_v, gpu_device), GuardedRBM(arena, W, b_h, b_v, gpu_device)
    B.freeze_params()
    ba = arena.carve_floats(NV, "b_A", data=b_a)
    arena.freeze(ba)
    v = (np.random.default_rng(3).random((ROWS, NV)) < 0.5).astype(np.float32)
    return A, B, arena, b_a, ba, v


def test_ais_step_guarded(gpu_device, pair):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    A, B, arena, b_a, ba, v = pair
    vb = arena.carve_matrix(ROWS, NV, data=v, name="v_in")          # wide ld, NaN padding, frozen
    a = A.ais_step(DeviceMatrix.from_host(v, gpu_device), 0.3, 0.4, 5, base_bias=b_a, chain0=6, seed=9)
    b = B.ais_step(vb, 0.3, 0.4, 5, base_bias=ba, chain0=6, seed=9)
    arena.check()
    A.check_status()
    for key in ("h", "prob_h", "u_h", "v", "prob_v", "u_v"):
        assert b[key].ld > a[key].ld, "the guarded outputs have wide leading dimensions"
        eq(a[key].view(), b[key].view(), key)
    eq(a["dlogw"], b["dlogw"], "dlogw")
    assert bool(torch.isfinite(b["dlogw"]).all().item())


def test_ais_run_guarded(gpu_device, pair):
    A, B, arena, b_a, ba, _ = pair
    la, va = A.ais_run(R.FREE_BETAS, ROWS, base_bias=b_a, chain0=6, seed=9, want_v=True)
    lb, vb = B.ais_run(R.FREE_BETAS, ROWS, base_bias=ba, chain0=6, seed=9, want_v=True)
    arena.check()
    A.check_status()
    assert vb.ld > va.ld
    eq(la.view(torch.float32), lb.view(torch.float32), "logw")
    eq(va.view(), vb.view(), "v_final")
    assert bool(torch.isfinite(lb).all().item())


def test_ais_short_workspace_refused(gpu_device, pair):
    _, B, arena, _, ba, v = pair
    lib, ctx = B.lib, B.ctx.handle
    need = int(lib.kurbm_ais_workspace_bytes(ctx, ROWS, NV, NH))
    assert need > 16
    ws = arena.carve(need - 16, "short_ws")
    vb = arena.carve_matrix(ROWS, NV, data=v, name="v_in")
    h, vo = arena.carve_matrix(ROWS, NH, name="h"), arena.carve_matrix(ROWS, NV, name="v_out")
    dlogw = arena.carve_floats(ROWS, "dlogw")
    logw = arena.carve_floats(2 * ROWS, "logw")
    betas = np.ascontiguousarray(R.FREE_BETAS)
    arena.freeze_all()
    code = lib.kurbm_ais_step(ctx, C.byref(B.params), ba.data_ptr(), 0.3, 0.4, 5, vb.ptr(), vb.ld, ROWS, 0, 9, dlogw.data_ptr(),
                              h.ptr(), h.ld, vo.ptr(), vo.ld, None, None, None, None, ws.data_ptr(), ws.numel(), B._stream())
    assert code == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    code = lib.kurbm_ais_run(ctx, C.byref(B.params), ba.data_ptr(), betas.ctypes.data_as(C.POINTER(C.c_double)), int(betas.size),
                             ROWS, 0, 9, logw.data_ptr(), vo.ptr(), vo.ld, ws.data_ptr(), ws.numel(), B._stream())
    assert code == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    arena.check()
