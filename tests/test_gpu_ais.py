"""GPU tier: the AIS kernels (kurbm_ais_step, kurbm_ais_run) against the float64 restatement of tests/ais_ref.py, and the
log-partition estimate against the exact value of a model small enough to enumerate."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # ais_ref.py lives beside this file
import ais_ref as R
from ais_ref import FLIP_BAND, TOL

pytestmark = pytest.mark.gpu


def rel_err(a, ref):
    return np.max(np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64))))


def _engine(W, b_h, b_v, device):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    return DeviceRBM(W, b_h, b_v, device)


def _wide(x, device):
    """x as a DeviceMatrix with a wide leading dimension whose padding is NaN."""
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix, round_up
    rows, cols = x.shape
    ld = round_up(cols, 4) + 8
    t = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=device)
    t[:, :cols].copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return DeviceMatrix(t, rows, cols, ld)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _step(gpu_device, params, v, beta_prev, beta, k, chain0, seed):
    W, b_h, b_v, b_a = params
    e = _engine(W, b_h, b_v, gpu_device)
    out = e.ais_step(_wide(v, gpu_device), beta_prev, beta, k, base_bias=b_a, chain0=chain0, seed=seed)
    torch.cuda.synchronize()
    e.check_status()
    return {key: (m.cpu().numpy() if isinstance(m, torch.Tensor) else m.to_numpy()) for key, m in out.items()}


# ---- 1. one temperature, teacher-forced ----------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.0, 0.1), (0.3, 0.4), (0.9, 1.0)])
@pytest.mark.parametrize("chain0", [0, 6])
@pytest.mark.parametrize("shape", [(37, 70, 36), (200, 70, 36), (130, 300, 200)])
def test_ais_step_against_restatement(gpu_device, shape, chain0, betas):
    """Shapes ragged against every tile size (the last with several column tiles in both launches); chain0 = 6 makes a lane's
    four rows straddle two Philox blocks; the input has a wide leading dimension with NaN padding."""
    rows, nv, nh = shape
    beta_prev, beta = betas
    k, seed = 3, 11
    params = W, b_h, b_v, b_a = R.normal_params(1000 + rows + nv, nv, nh, 0.3, 0.3)
    v = (np.random.default_rng(rows).random((rows, nv)) < 0.5).astype(np.float32)
    out = _step(gpu_device, params, v, beta_prev, beta, k, chain0, seed)

    ph, uh, h_ref = R.hidden(W, b_h, beta, k, v, chain0, seed)
    assert np.array_equal(_bits(out["u_h"]), _bits(uh)), "hidden uniforms must be bit-exact"
    assert np.max(np.abs(out["prob_h"] - ph)) <= TOL
    assert np.array_equal(out["h"], (out["u_h"] < out["prob_h"]).astype(np.float32)), "h must be (u < p) of the GPU's own p"
    differ = out["h"] != h_ref
    assert np.all(np.abs(uh - ph)[differ] <= FLIP_BAND), "h differs from the restatement outside the rounding band"

    # v_out is drawn from the GPU's own h: the restatement is fed that h
    pv, uv, v_ref = R.visible(W, b_v, b_a, beta, k, out["h"], chain0, seed)
    assert np.array_equal(_bits(out["u_v"]), _bits(uv)), "visible uniforms must be bit-exact"
    assert np.max(np.abs(out["prob_v"] - pv)) <= TOL
    assert np.array_equal(out["v"], (out["u_v"] < out["prob_v"]).astype(np.float32)), "v must be (u < p) of the GPU's own p"
    differ = out["v"] != v_ref
    assert np.all(np.abs(uv - pv)[differ] <= FLIP_BAND), "v differs from the restatement outside the rounding band"

    d_ref, mag = R.delta(W, b_h, b_v, b_a, beta_prev, beta, v)
    err = np.abs(out["dlogw"].astype(np.float64) - d_ref)
    print("max |Delta_gpu - Delta_ref| / max(1, magnitude) = %.3g" % np.max(err / np.maximum(1.0, mag)))
    assert np.all(err <= TOL * np.maximum(1.0, mag))


def test_ais_step_every_tile_shape_bit_identical(gpu_device):
    """The eight tile shapes of both launches (KURBM_CFG_VH / KURBM_CFG_HV force one): the row partials are kept per group of 16
    columns whatever the tile, so Delta and the samples are bit for bit those of the planner's own choice."""
    from keras_unsupervised_amd._lib import Context
    rows, nv, nh = 130, 300, 200
    params = R.normal_params(9, nv, nh, 0.3, 0.3)
    v = (np.random.default_rng(9).random((rows, nv)) < 0.5).astype(np.float32)
    want = _step(gpu_device, params, v, 0.3, 0.4, 2, 6, 5)
    ctx = Context.get(gpu_device.index)
    try:
        for cfg in range(8):
            ctx.set_option("KURBM_CFG_VH", cfg)
            ctx.set_option("KURBM_CFG_HV", cfg)
            got = _step(gpu_device, params, v, 0.3, 0.4, 2, 6, 5)
            for key in want:
                assert np.array_equal(_bits(got[key]), _bits(want[key])), "tile shape %d: %s differs" % (cfg, key)
    finally:
        ctx.set_option("KURBM_CFG_VH", -1)
        ctx.set_option("KURBM_CFG_HV", -1)


# ---- 2. the same call at the spacing of a long run -------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.5, 0.5001), (0.0, 0.0001), (0.9999, 1.0)])
def test_ais_step_delta_at_fine_spacing(gpu_device, betas):
    """d beta = 1e-4 with pre-activations a ~ N(0, 3) (W ~ N(0, 3 / sqrt(35)) under half-on visibles of 70 units).  The bar is
    relative to the UN-cancelled magnitude, without max(1, .): the literal difference of two fp32 softplus values misses it
    (2-4e-4), log1p(sigmoid(beta_prev a) expm1(dbeta a)) meets it."""
    rows, nv, nh = 200, 70, 36
    beta_prev, beta = betas
    W, b_h, b_v, b_a = R.normal_params(77, nv, nh, 3.0 / np.sqrt(35.0), 0.3)
    v = (np.random.default_rng(5).random((rows, nv)) < 0.5).astype(np.float32)
    out = _step(gpu_device, (W, b_h, b_v, b_a), v, beta_prev, beta, 1234, 0, 21)
    d_ref, mag = R.delta(W, b_h, b_v, b_a, beta_prev, beta, v)
    err = np.abs(out["dlogw"].astype(np.float64) - d_ref)
    print("max |Delta_gpu - Delta_ref| / magnitude = %.3g" % np.max(err / mag))
    assert np.all(err <= TOL * mag)


# ---- 3. a short free run, chain by chain ---------------------------------------------------------------------------------
def _free_run_gpu(gpu_device, seed, n_chains=R.FREE_CHAINS, chain0=0):
    W, b_h, b_v, b_a = R.free_params(seed)
    e = _engine(W, b_h, b_v, gpu_device)
    logw, vf = e.ais_run(R.FREE_BETAS, n_chains, base_bias=b_a, chain0=chain0, seed=seed, want_v=True)
    torch.cuda.synchronize()
    e.check_status()
    return logw.cpu().numpy(), vf.to_numpy()


@pytest.mark.parametrize("seed", [7, 8])
def test_ais_run_against_restatement(gpu_device, seed):
    logw, vf = _free_run_gpu(gpu_device, seed)
    logw_ref, v_ref, flagged = R.free_run(seed)
    print("flagged chains: %d of %d" % (flagged.sum(), flagged.size))
    assert flagged.sum() <= 0.10 * flagged.size
    ok = ~flagged
    print("rel_err(logw) over the unflagged chains = %.3g" % rel_err(logw[ok], logw_ref[ok]))
    assert rel_err(logw[ok], logw_ref[ok]) <= TOL
    assert np.array_equal(vf[ok], v_ref[ok].astype(np.float32))


def test_ais_run_reproducible_and_chain0(gpu_device):
    a, va = _free_run_gpu(gpu_device, 7)
    b, vb = _free_run_gpu(gpu_device, 7)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(va, vb), "one seed, two runs: bit-identical"
    c, _ = _free_run_gpu(gpu_device, 8)
    assert not np.array_equal(a, c), "another seed must give other weights"
    t, vt = _free_run_gpu(gpu_device, 7, n_chains=136, chain0=64)
    assert np.array_equal(t.view(np.uint64), a[64:].view(np.uint64)), "chain0 = 64 must reproduce chains 64 .. 199 bit for bit"
    assert np.array_equal(vt, va[64:])


def test_ais_refuses_bad_arguments(gpu_device):
    from keras_unsupervised_amd._lib import KurbmError
    W, b_h, b_v, b_a = R.free_params(7)
    e = _engine(W, b_h, b_v, gpu_device)
    for betas in ([0.0, 0.5], [0.1, 1.0], [0.0, 0.5, 0.5, 1.0], [0.0, 0.6, 0.4, 1.0], [1.0]):
        with pytest.raises(KurbmError, match="betas"):
            e.ais_run(betas, 8, base_bias=b_a)
    short = torch.zeros(int(e.lib.kurbm_ais_workspace_bytes(e.ctx.handle, 8, e.n_vis, e.n_hid)) - 16, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(KurbmError, match="workspace too small"):
        e.ais_run([0.0, 1.0], 8, base_bias=b_a, ws=short)


# ---- 4. the estimate against the truth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_log_partition_against_exact(gpu_device, seed):
    """13 x 11, 256 chains, 500 linear temperatures.  The margin is five standard errors of the CPU restatement's weights for the
    same seed (the GPU's chains part from the restatement after a rounding-band flip and are then a fresh sample of the same
    estimator); the restatement itself must sit within three of them, so a broken yardstick cannot widen the margin."""
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM, ais
    W, b_h, b_v, b_a = R.est_params(seed)
    nv, nh = R.EST_SHAPE
    exact = ais.exact_log_partition(W, b_h, b_v)
    assert abs(exact - R.brute_force_log_z(W, b_h, b_v)) <= 1e-9
    z_ref, se_ref, _ = R.est_run(seed)
    assert abs(z_ref - exact) <= 3.0 * se_ref

    e = _engine(W, b_h, b_v, gpu_device)
    betas = ais.beta_schedule(R.EST_TEMPS)
    logw, _ = e.ais_run(betas, R.EST_CHAINS, base_bias=b_a, seed=seed)
    z_gpu, se_gpu, _ = ais.estimate(logw.cpu().numpy(), b_a, nh)
    print("seed %d: exact %.6f, gpu %.6f (error %+.4f), restatement error %+.4f, SE_ref %.4f, SE_gpu %.4f"
          % (seed, exact, z_gpu, z_gpu - exact, z_ref - exact, se_ref, se_gpu))
    assert abs(z_gpu - exact) <= 5.0 * se_ref

    rbm = RBM({"batch_size": 16, "epochs": 1, "lr": 0.01}, nh, mode=MODE_VISIBLE_BERNOULLI, seed=seed, weights=(W, b_h, b_v),
              device=gpu_device)
    rbm.build((None, nv))
    before = (rbm._update_count, rbm._call_count)
    z_rbm = rbm.log_partition(n_chains=R.EST_CHAINS, betas=R.EST_TEMPS, base_rates=b_a)
    assert z_rbm == z_gpu, "RBM.log_partition must return the engine path's number"
    assert rbm.last_ais["log_z"] == z_gpu and rbm.last_ais["n_chains"] == R.EST_CHAINS and rbm.last_ais["n_betas"] == R.EST_TEMPS + 1
    assert np.array_equal(rbm.last_ais["logw"], logw.cpu().numpy())
    assert se_ref / 2.0 <= rbm.last_ais["stderr"] <= 2.0 * se_ref
    assert abs(rbm.log_partition(method="exact") - exact) <= 1e-9

    V = (np.random.default_rng(seed).random((50, nv)) < 0.5).astype(np.float32)
    F = e.free_energy(_wide(V, gpu_device), 50).double().cpu().numpy()
    assert abs(rbm.log_likelihood(V, log_z=z_gpu) - float(-F.mean() - z_gpu)) <= 1e-9
    rbm.log_partition(n_chains=R.EST_CHAINS, betas=R.EST_TEMPS, base_rates=b_a)
    assert abs(rbm.log_likelihood(V) - float(-F.mean() - z_gpu)) <= 1e-9, "the cached log Z"
    assert (rbm._update_count, rbm._call_count) == before
    assert np.array_equal(rbm.rbm_weight, W)
