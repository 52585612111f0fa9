"""GPU tier: Gibbs runs (kurbm_gibbs_run, RBM.gibbs / sample, DBN.sample) against the float64 restatement of
tests/gibbs_ref.py, and the samples of a model small enough to enumerate against its exact distribution."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # gibbs_ref.py lives beside this file
import gibbs_ref as R
from gibbs_ref import TOL

pytestmark = pytest.mark.gpu

BERN, GAUSS = R.MODE_BERNOULLI, R.MODE_GAUSSIAN
KURBM_ERR_ARG, KURBM_ERR_WORKSPACE = -1, -4


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


def _run(device, params, v0, chain0, seed, mode=BERN, burn_in=1, thin=1, n_keep=1, clamp=None, engine=None):
    """(v [n_keep, rows, n_vis], prob likewise) of one kurbm_gibbs_run from a wide, NaN-padded start."""
    e = engine or _engine(*params, device)
    v, p = e.gibbs_run(_wide(v0, device), burn_in=burn_in, thin=thin, n_keep=n_keep, chain0=chain0, seed=seed, mode=mode,
                       clamp=clamp, want_prob=True)
    torch.cuda.synchronize()
    e.check_status()
    shape = (n_keep, v0.shape[0], v0.shape[1])
    return v.to_numpy().reshape(shape), p.to_numpy().reshape(shape)


def _compare(v, p, ref, mode=BERN, what=""):
    """Every kept plane against the restatement on the unflagged chains; at most 10 % of the chains may be flagged."""
    v_ref, p_ref, flagged = ref
    assert flagged.sum() <= 0.10 * flagged.size, "%s: %d of %d chains flagged" % (what, flagged.sum(), flagged.size)
    ok = ~flagged
    assert v.shape == v_ref.shape and p.shape == p_ref.shape
    if mode == BERN:
        assert set(np.unique(v)) <= {0.0, 1.0}
        assert np.array_equal(v[:, ok], v_ref[:, ok]), "%s: an unflagged chain differs from the restatement" % what
        err = np.max(np.abs(p[:, ok] - p_ref[:, ok]))
        print("%s: %d flagged; max |prob - ref| = %.3g" % (what, int(flagged.sum()), err))
        assert err <= TOL
    else:
        ev = np.max(np.abs(v[:, ok] - v_ref[:, ok]) / np.maximum(1.0, np.abs(v_ref[:, ok])))
        ep = np.max(np.abs(p[:, ok] - p_ref[:, ok]) / np.maximum(1.0, np.abs(p_ref[:, ok])))
        print("%s: %d flagged; max |v - v_ref| / max(1, |v_ref|) = %.3g, of the means %.3g" % (what, int(flagged.sum()), ev, ep))
        assert ev <= TOL and ep <= TOL


# ---- 1. free runs against the restatement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain8(gpu_device):
    """The plain eight-sweep run of both seeds, shared by the tests that compare against it."""
    return {seed: _run(gpu_device, R.free_params(seed), R.free_init(seed), 0, seed, burn_in=R.FREE_SWEEPS) for seed in (7, 8)}


@pytest.mark.parametrize("seed", [7, 8])
def test_free_run_against_restatement(gpu_device, plain8, seed):
    v, p = plain8[seed]
    _compare(v, p, R.free_run(seed), what="free run, seed %d" % seed)


@pytest.mark.parametrize("seed", [7, 8])
def test_kept_samples(gpu_device, plain8, seed):
    """burn_in 2, thin 3, n_keep 3: sweeps 2, 5 and 8; the last kept plane is the plain run's, bit for bit."""
    v, p = _run(gpu_device, R.free_params(seed), R.free_init(seed), 0, seed, burn_in=2, thin=3, n_keep=3)
    _compare(v, p, R.free_run(seed, 2, 3, 3), what="kept samples, seed %d" % seed)
    assert np.array_equal(_bits(v[2]), _bits(plain8[seed][0][0])) and np.array_equal(_bits(p[2]), _bits(plain8[seed][1][0]))
    assert not np.array_equal(v[0], v[2])


@pytest.mark.parametrize("seed", [7, 8])
def test_clamped_run(gpu_device, seed):
    """Columns {0, 5, 63, 64, 69} straddle a 64-group of the k-permuted byte plane; given once as indices, once as a mask."""
    v0 = R.free_init(seed)
    mask = np.zeros(R.FREE_SHAPE[0], dtype=bool)
    mask[R.CLAMP_COLS] = True
    for clamp in (R.CLAMP_COLS.tolist(), mask):
        v, p = _run(gpu_device, R.free_params(seed), v0, 0, seed, burn_in=2, thin=3, n_keep=3, clamp=clamp)
        for j in range(3):
            assert np.array_equal(_bits(v[j][:, R.CLAMP_COLS]), _bits(v0[:, R.CLAMP_COLS])), "kept plane %d: clamped samples" % j
            assert np.array_equal(_bits(p[j][:, R.CLAMP_COLS]), _bits(v0[:, R.CLAMP_COLS])), "kept plane %d: clamped probs" % j
        _compare(v, p, R.free_run(seed, 2, 3, 3, True), what="clamped run, seed %d" % seed)


def test_clamped_real_valued_start(gpu_device):
    """Bernoulli visibles with REAL clamped values (grey pixels): the clamped units enter the products as their three exact
    pieces, the free ones as 0/1."""
    seed = 7
    W, b_h, b_v = R.free_params(seed)
    v0 = R.free_init(seed)[:64].copy()
    v0[:, R.CLAMP_COLS] = np.random.default_rng(1).random((64, R.CLAMP_COLS.size)).astype(np.float32)
    v, p = _run(gpu_device, (W, b_h, b_v), v0, 0, seed, burn_in=4, clamp=R.CLAMP_COLS)
    assert np.array_equal(_bits(v[0][:, R.CLAMP_COLS]), _bits(v0[:, R.CLAMP_COLS]))
    ref = R.run(W, b_h, b_v, v0, 0, seed, BERN, 4, 1, 1, R.CLAMP_COLS)
    free = np.setdiff1d(np.arange(R.FREE_SHAPE[0]), R.CLAMP_COLS)
    ok = ~ref[2]
    assert ok.sum() >= 0.9 * ok.size
    assert np.array_equal(v[0][ok][:, free], ref[0][0][ok][:, free]) and np.max(np.abs(p[0][ok] - ref[1][0][ok])) <= TOL


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv,nh,chain0,sweeps", [(130, 300, 200, 0, 3), (1, 70, 36, 0, 3), (5, 70, 36, 0, 3), (37, 70, 36, 64, 3)])
def test_shapes(gpu_device, rows, nv, nh, chain0, sweeps):
    """130 x 300 x 200: several tiles in both launches, ragged against every tile size; one chain and five; chain0 = 64."""
    seed = 21
    W, b_h, b_v = R.normal_params(600 + rows + nv, nv, nh, 0.3, 0.3)
    v0 = (np.random.default_rng(rows).random((rows, nv)) < 0.5).astype(np.float32)
    clamp = [0, nv // 2, nv - 1]
    for cl in (None, clamp):
        v, p = _run(gpu_device, (W, b_h, b_v), v0, chain0, seed, burn_in=sweeps, clamp=cl)
        v_ref, p_ref, flagged = R.run(W, b_h, b_v, v0, chain0, seed, BERN, sweeps, 1, 1, cl)
        ok = ~flagged
        assert flagged.sum() <= 0.10 * rows
        assert np.array_equal(v[0][ok], v_ref[0][ok]) and np.max(np.abs(p[0][ok] - p_ref[0][ok])) <= TOL


# ---- 3. Gaussian visibles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamped", [False, True])
def test_gaussian_run(gpu_device, clamped):
    seed = 7
    v0 = R.gauss_init(seed)
    v, p = _run(gpu_device, R.gauss_params(seed), v0, 0, seed, mode=GAUSS, burn_in=R.GAUSS_SWEEPS,
                clamp=R.CLAMP_COLS if clamped else None)
    _compare(v, p, R.gauss_run(seed, clamped), mode=GAUSS, what="Gaussian run%s" % (", clamped" if clamped else ""))
    if clamped:
        assert np.array_equal(_bits(v[0][:, R.CLAMP_COLS]), _bits(v0[:, R.CLAMP_COLS]))
        assert np.array_equal(_bits(p[0][:, R.CLAMP_COLS]), _bits(v0[:, R.CLAMP_COLS]))


# ---- 4. reproducibility and the draws ---------------------------------------------------------------------------------------
def test_reproducible_and_seeded(gpu_device, plain8):
    again = _run(gpu_device, R.free_params(7), R.free_init(7), 0, 7, burn_in=R.FREE_SWEEPS)
    assert np.array_equal(_bits(again[0]), _bits(plain8[7][0])) and np.array_equal(_bits(again[1]), _bits(plain8[7][1]))
    other = _run(gpu_device, R.free_params(7), R.free_init(7), 0, 70, burn_in=R.FREE_SWEEPS)
    assert not np.array_equal(other[0], plain8[7][0])
    moved = _run(gpu_device, R.free_params(7), R.free_init(7), 4, 7, burn_in=R.FREE_SWEEPS)
    assert not np.array_equal(moved[0], plain8[7][0])


@pytest.mark.parametrize("chain0", [0, 64])
def test_one_sweep_uses_the_contract_uniforms(gpu_device, chain0):
    """A T = 1 run, teacher-forced: the x3 half-step hook with the run's counters (sites GIBBS_H / GIBBS_V, step 1, row0 =
    chain0) returns its uniforms -- those of oracle.philox -- and its states; the run's sample must be [u < p] of the run's own
    probabilities under exactly those uniforms, and its probabilities those of the hook's hidden states."""
    from keras_unsupervised_amd import _lib
    seed, rows = 13, 200
    W, b_h, b_v = R.free_params(7)
    v0 = R.free_init(7)
    e = _engine(W, b_h, b_v, gpu_device)
    v, p = _run(gpu_device, None, v0, chain0, seed, burn_in=1, engine=e)
    x = _wide(v0, gpu_device)
    hh = e.half_step_bf16("vh", x, rows, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, seed, R.STREAM_GIBBS_H, 1, row0=chain0, pieces=3)
    hv = e.half_step_bf16("hv", hh["sample"], rows, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, seed, R.STREAM_GIBBS_V, 1, row0=chain0,
                          pieces=3)
    torch.cuda.synchronize()
    uh, uv = hh["u"].to_numpy(), hv["u"].to_numpy()
    assert np.array_equal(_bits(uh), _bits(R.uniform(rows, 36, seed, R.STREAM_GIBBS_H, 1, chain0)))
    assert np.array_equal(_bits(uv), _bits(R.uniform(rows, 70, seed, R.STREAM_GIBBS_V, 1, chain0)))
    assert np.array_equal(v[0], (uv < p[0]).astype(np.float32)), "v must be [u < p] of the run's own p under the contract's uniforms"
    assert np.max(np.abs(p[0] - hv["prob"].to_numpy())) <= TOL, "the run's hidden states are not those of the contract's uniforms"


# ---- 5. the distribution ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamped", [False, True])
def test_samples_follow_the_enumerated_distribution(gpu_device, clamped):
    """6 x 5, 8192 chains, 200 sweeps; 5 sigma where the restatement's own check (CPU tier) uses 4: after any flip the GPU's
    chains are a fresh sample."""
    W, b_h, b_v = R.dist_params()
    cl = R.DIST_CLAMP if clamped else None
    pdist = R.exact_pv(W, b_h, b_v, *((R.DIST_CLAMP, R.DIST_VALUES) if clamped else ()))
    v, _ = _run(gpu_device, (W, b_h, b_v), R.dist_init(clamped), 0, 5, burn_in=R.DIST_BURN, clamp=cl)
    bad, f = R.band_violations(v[0], pdist, 5.0)
    print("max |f - p| = %.4f over 64 states" % np.max(np.abs(f - pdist)))
    assert bad.size == 0, "states %s: f = %s, p = %s" % (bad, f[bad], pdist[bad])
    if clamped:
        assert np.all(v[0][:, 0] == 1.0) and np.all(v[0][:, 3] == 0.0)


# ---- 6. the public surface ----------------------------------------------------------------------------------------------------
HPS = {"batch_size": 64, "epochs": 1, "lr": 0.01}


def _rbm(device, seed=3, mode=BERN, shape=R.FREE_SHAPE, pseed=7):
    from keras_unsupervised_amd.ebm import RBM
    W, b_h, b_v = R.normal_params(300 + pseed, shape[0], shape[1], 0.3, 0.3)
    r = RBM(HPS, shape[1], mode=mode, seed=seed, weights=(W, b_h, b_v), device=device)
    r.build((None, shape[0]))
    return r


@pytest.mark.parametrize("mode", [BERN, GAUSS])
def test_rbm_gibbs_and_sample(gpu_device, mode):
    r = _rbm(gpu_device, mode=mode)
    W0 = r.get_weights()
    v0 = R.free_init(7)[:50] if mode == BERN else R.gauss_init(7)[:50]
    a, pa = r.gibbs(v0, n_steps=3, clamp=[1, 64], return_prob=True)          # chains 0 .. 49
    b = r.sample(10, n_chains=4, burn_in=5, thin=2)                          # chain0 = 52
    c = r.sample(10, n_chains=4, burn_in=5, thin=2)                          # chain0 = 56
    assert isinstance(a, np.ndarray) and a.shape == pa.shape == (50, 70) and b.shape == c.shape == (10, 70)
    assert not np.array_equal(b, c), "a second sample() call must take fresh chains"
    assert r._chains_used == 60 and r._update_count == 0 and r._call_count == 0 and r.last_ais is None
    for x, y in zip(W0, r.get_weights()):
        assert np.array_equal(x, y)
    # the engine path with the same counters gives the same bits
    e = r._dev
    ea, epa = e.gibbs_run(_wide(v0, gpu_device), burn_in=3, chain0=0, seed=3, mode=mode, clamp=[1, 64], want_prob=True)
    assert np.array_equal(_bits(ea.to_numpy()), _bits(a)) and np.array_equal(_bits(epa.to_numpy()), _bits(pa))
    eb, _ = e.gibbs_run(r._start_chains(4, 52, 3), burn_in=5, thin=2, n_keep=3, chain0=52, seed=3, mode=mode)
    assert np.array_equal(_bits(eb.to_numpy()[:10]), _bits(b))
    if mode == BERN:
        assert set(np.unique(b)) <= {0.0, 1.0}
        u = R.uniform(4, 70, 3, R.STREAM_GIBBS_V, 0, 52)
        want = (u < R.sigmoid(W0[2].astype(np.float64))[None, :]).astype(np.float32)
        near = np.abs(u - R.sigmoid(W0[2].astype(np.float64))[None, :]) <= R.FLIP_BAND
        assert np.array_equal(r._start_chains(4, 52, 3).to_numpy()[~near], want[~near])
    # a rebuilt object replays both calls
    r2 = _rbm(gpu_device, mode=mode)
    a2 = r2.gibbs(torch.from_numpy(v0).to(gpu_device), n_steps=3, clamp=[1, 64])
    assert isinstance(a2, torch.Tensor) and a2.device.type == "cuda" and np.array_equal(_bits(a2.cpu().numpy()), _bits(a))
    assert np.array_equal(_bits(r2.sample(10, n_chains=4, burn_in=5, thin=2)), _bits(b))
    assert np.array_equal(_bits(r2.sample(10, n_chains=4, burn_in=5, thin=2)), _bits(c))


@pytest.mark.parametrize("rows", [50, 1030])
def test_probs_are_the_half_steps_probability_planes(gpu_device, rows):
    """hidden_probs / visible_probs: NOISE_NONE on the existing half steps (the x3 route from 1024 rows on), no counter used."""
    from keras_unsupervised_amd import _lib
    r = _rbm(gpu_device)
    W, b_h, b_v = r.get_weights()
    v = (np.random.default_rng(rows).random((rows, 70)) < 0.5).astype(np.float32)
    h = (np.random.default_rng(rows + 1).random((rows, 36)) < 0.5).astype(np.float32)
    ph, pv = r.hidden_probs(v), r.visible_probs(h)
    assert r._call_count == 0 and isinstance(ph, np.ndarray)
    assert np.max(np.abs(ph - R.sigmoid(v.astype(np.float64) @ W + b_h))) <= TOL
    assert np.max(np.abs(pv - R.sigmoid(h.astype(np.float64) @ W.T + b_v))) <= TOL
    e = r._dev
    x = _wide(v, gpu_device)
    if rows < 1024:
        want = e.half_step("vh", x, rows, 0, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, 3, 0x100, 0, want_prob=True)["prob"]
    else:
        want = e.half_step_bf16("vh", x, rows, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, 3, 0x100, 0, pieces=3)["prob"]
    assert np.array_equal(_bits(want.to_numpy()), _bits(ph)), "hidden_probs is the probability plane of the sampling half step"
    t = r.transform(v)[0]
    assert r._call_count == 1 and set(np.unique(t)) <= {0.0, 1.0}


def test_dbn_sample_and_transform_probs(gpu_device):
    from keras_unsupervised_amd.ebm import DBN
    def make():
        d = DBN()
        d.add_stack(_rbm(gpu_device, seed=3, shape=(70, 36), pseed=7))
        d.add_stack(_rbm(gpu_device, seed=4, shape=(36, 20), pseed=8))
        return d
    dbn = make()
    out = dbn.sample(12, burn_in=6, thin=2, n_chains=5)
    assert isinstance(out, np.ndarray) and out.shape == (12, 70) and set(np.unique(out)) <= {0.0, 1.0}
    # the manual composition with the same counters
    man = make()
    bottom, top = man._layers()
    h = top.sample(12, n_chains=5, burn_in=6, thin=2)
    assert np.array_equal(_bits(bottom.inv_transform(h)[0]), _bits(out))
    probs = make().sample(12, burn_in=6, thin=2, n_chains=5, return_prob=True)
    assert np.array_equal(_bits(probs), _bits(bottom.visible_probs(h))) and probs.min() >= 0.0 and probs.max() <= 1.0
    # init is carried up through transform first
    V = R.free_init(7)[:5]
    a = make().sample(5, burn_in=2, init=V)
    man = make()
    bottom, top = man._layers()
    b = bottom.inv_transform(top.sample(5, burn_in=2, init=bottom.transform(V)[0]))[0]
    assert np.array_equal(_bits(a), _bits(b))
    # transform_probs: hidden_probs through the layers
    tp = dbn.transform_probs(V)
    assert np.array_equal(_bits(tp), _bits(top.hidden_probs(bottom.hidden_probs(V)))) and tp.shape == (5, 20)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(gpu_device):
    from keras_unsupervised_amd import _lib
    rows, nv, nh = 12, 70, 36
    W, b_h, b_v = R.free_params(7)
    e = _engine(W, b_h, b_v, gpu_device)
    lib, ctx = e.lib, e.ctx.handle
    v0 = torch.zeros((rows, 72), dtype=torch.float32, device=gpu_device)
    out = torch.full((3 * rows * 72 + 8,), 7.0, dtype=torch.float32, device=gpu_device)
    prob = torch.full((3 * rows * 72 + 8,), 7.0, dtype=torch.float32, device=gpu_device)
    mask = torch.zeros(nv, dtype=torch.uint8, device=gpu_device)
    mir = e.mirror(3)
    vp = 1 | _lib.V_BINARY
    need = int(lib.kurbm_gibbs_workspace_bytes(ctx, rows, nv, nh, vp, BERN))
    assert need > 16 and lib.kurbm_gibbs_workspace_bytes(ctx, rows, nv, nh, 2, BERN) == 0
    assert lib.kurbm_gibbs_workspace_bytes(ctx, 0, nv, nh, vp, BERN) == 0 and lib.kurbm_gibbs_workspace_bytes(ctx, rows, nv, nh, vp, 2) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu_device)
    good = dict(mirror=mir.data_ptr(), mirror_bytes=mir.numel(), v_init=v0.data_ptr(), v_pieces=vp, ldv=72, n_chains=rows, chain0=0,
                seed=1, mode=BERN, burn_in=2, thin=2, n_keep=3, clamp=mask.data_ptr(), v_out=out.data_ptr(), prob_out=prob.data_ptr(),
                ldo=72, keep_stride=rows * 72, ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.kurbm_gibbs_run(ctx, C.byref(e.params), a["mirror"], a["mirror_bytes"], a["v_init"], a["v_pieces"], a["ldv"],
                                   a["n_chains"], a["chain0"], a["seed"], a["mode"], a["burn_in"], a["thin"], a["n_keep"], a["clamp"],
                                   a["v_out"], a["prob_out"], a["ldo"], a["keep_stride"], a["ws"], a["ws_bytes"], e._stream())

    bad = [dict(v_init=None), dict(v_init=v0.data_ptr() + 4), dict(v_out=None), dict(v_out=out.data_ptr() + 4),
           dict(prob_out=prob.data_ptr() + 4), dict(mirror=None), dict(ws=None), dict(ws=ws.data_ptr() + 4),
           dict(ldv=68), dict(ldv=74), dict(ldo=68), dict(ldo=74), dict(keep_stride=rows * 72 - 4), dict(keep_stride=rows * 72 + 2),
           dict(n_chains=0), dict(burn_in=0), dict(thin=0), dict(n_keep=0), dict(chain0=2), dict(v_pieces=2), dict(v_pieces=0),
           dict(mode=2)]
    for kw in bad:
        assert call(**kw) == KURBM_ERR_ARG, "not refused: %s" % (kw,)
    assert call(ws_bytes=need - 16) == KURBM_ERR_WORKSPACE and b"workspace too small" in lib.kurbm_last_error()
    assert call(mirror_bytes=mir.numel() - 16) == KURBM_ERR_WORKSPACE and b"mirror too small" in lib.kurbm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all().item()) and bool((prob == 7.0).all().item()), "a refused call wrote an output"
    assert call() == 0                                  # ... and the same arguments, unspoiled, run
    assert call(n_keep=1, keep_stride=0) == 0           # (keep_stride is not looked at for one kept sample)
    torch.cuda.synchronize()
    got = out[: 3 * rows * 72].view(3, rows, 72)
    assert bool(((got[:, :, :nv] == 0.0) | (got[:, :, :nv] == 1.0)).all().item()) and bool((got[:, :, nv:] == 7.0).all().item())
    assert bool((out[3 * rows * 72:] == 7.0).all().item())
    e.check_status()
