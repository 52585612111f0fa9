"""GPU tier of the free label blocks: kurbm_gibbs_run_labels, kurbm_ais_step_labels / kurbm_ais_run_labels and the public calls
built on them (RBM.gibbs / sample / log_partition / log_likelihood with label='free', DBN.sample) against the float64 restatement
of tests/labelsite_ref.py, and against the enumerated joint distribution of a model small enough to enumerate.
tests/test_labelsite_host.py holds the restatement itself, and the flag rates of the fixtures, to account on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # the *_ref.py modules live beside this file
import ais_ref as A
import labels_ref as L
import labelsite_ref as S
from labelsite_ref import FLIP_BAND, TOL

pytestmark = pytest.mark.gpu

HPS = {"batch_size": 16, "epochs": 1, "lr": 0.01}


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


def _np(out):
    return {key: (m.cpu().numpy() if isinstance(m, torch.Tensor) else m.to_numpy()) for key, m in out.items() if m is not None}


@pytest.fixture
def ctx_option(gpu_device):
    """Set experiment knobs on the device's context for one test (kurbm_ctx_set_option); restored afterwards."""
    from keras_unsupervised_amd._lib import Context
    ctx = Context.get(gpu_device.index)
    touched = {}

    def set_option(name, value, default):
        touched[name] = default
        ctx.set_option(name, value)

    yield set_option
    for name, default in touched.items():
        ctx.set_option(name, default)


# ---- 1. Gibbs runs with a free block ------------------------------------------------------------------------------------------
def _run(device, i, kind, chain0=0):
    """(v [n_keep, rows, n_vis], prob likewise) of one kurbm_gibbs_run_labels on fixture (i, kind) from a wide, NaN-padded start."""
    params, v0, clamp, kw, _ = S.gibbs_fixture(i, kind, chain0)
    e = _engine(*params, device)
    v, p = e.gibbs_run(_wide(v0, device), chain0=chain0, seed=S.GIBBS_SEED, clamp=clamp, want_prob=True, n_labels=S.GIBBS_SHAPES[i][2], **kw)
    torch.cuda.synchronize()
    e.check_status()
    shape = (kw["n_keep"], v0.shape[0], v0.shape[1])
    return v.to_numpy().reshape(shape), p.to_numpy().reshape(shape)


def _compare(v, p, i, kind, chain0=0, what=""):
    """_compare's rule of tests/test_gpu_gibbs.py: on the unflagged chains every kept plane equals the restatement and its
    probabilities lie within 1e-4; at most 10 % of the chains are flagged.  And the block of EVERY chain is one-hot, its
    probabilities a distribution; clamped columns carry the start's bits."""
    _, v0, clamp, _, (v_ref, p_ref, flagged) = S.gibbs_fixture(i, kind, chain0)
    n_pix = S.GIBBS_SHAPES[i][1]
    assert flagged.sum() <= 0.10 * flagged.size, "%s: %d of %d chains flagged" % (what, flagged.sum(), flagged.size)
    ok = ~flagged
    assert v.shape == v_ref.shape and p.shape == p_ref.shape
    free = np.ones(v.shape[2], dtype=bool)
    if clamp is not None:
        free[clamp] = False
        for j in range(v.shape[0]):
            assert np.array_equal(_bits(v[j][:, clamp]), _bits(v0[:, clamp])) and np.array_equal(_bits(p[j][:, clamp]), _bits(v0[:, clamp]))
    assert set(np.unique(v[:, :, free])) <= {0.0, 1.0}
    assert np.array_equal(v[:, :, n_pix:].sum(axis=2), np.ones(v.shape[:2])), "%s: a block that is not one-hot" % what
    assert np.max(np.abs(p[:, :, n_pix:].sum(axis=2) - 1.0)) <= 1e-5
    assert np.array_equal(v[:, ok], v_ref[:, ok].astype(np.float32)), "%s: an unflagged chain differs from the restatement" % what
    err = np.max(np.abs(p[:, ok] - p_ref[:, ok]))
    print("%s: %d flagged; max |prob - ref| = %.3g" % (what, int(flagged.sum()), err))
    assert err <= TOL


@pytest.fixture(scope="module")
def free8(gpu_device):
    """The free eight-sweep run of every fixture, shared by the tests that compare against it."""
    return {i: _run(gpu_device, i, "free") for i in range(len(S.GIBBS_SHAPES))}


@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_free_run_against_restatement(gpu_device, free8, i):
    v, p = free8[i]
    _compare(v, p, i, "free", what="free run %s" % (S.GIBBS_SHAPES[i],))
    v2, p2 = _run(gpu_device, i, "free")
    assert np.array_equal(_bits(v), _bits(v2)) and np.array_equal(_bits(p), _bits(p2)), "the same call twice: identical bits"


@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_kept_samples(gpu_device, free8, i):
    """burn_in 2, thin 3, n_keep 3: sweeps 2, 5 and 8; the last kept plane is the free run's, bit for bit."""
    v, p = _run(gpu_device, i, "keep")
    _compare(v, p, i, "keep", what="kept samples %s" % (S.GIBBS_SHAPES[i],))
    assert np.array_equal(_bits(v[2]), _bits(free8[i][0][0])) and np.array_equal(_bits(p[2]), _bits(free8[i][1][0]))
    assert not np.array_equal(v[0], v[2])


@pytest.mark.parametrize("kind", ["clamp", "real"])
@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_pixels_clamped_across_the_blocks_group(gpu_device, i, kind):
    """Clamped pixels in the 8-byte group the block starts in: 0/1 values (the byte plane) and real ones (the bf16-piece plane,
    where the site writes hi = 1.0 / 0 and zero mid / lo pieces)."""
    v, p = _run(gpu_device, i, kind)
    _compare(v, p, i, kind, what="%s %s" % (kind, S.GIBBS_SHAPES[i]))


@pytest.mark.parametrize("kind", ["free", "clamp"])
@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_bf16_hidden_plane(gpu_device, ctx_option, free8, i, kind):
    """KURBM_X3_BYTES=0: the hidden plane is one bf16 piece and so is the visible one; the same numbers, bit for bit."""
    ctx_option("KURBM_X3_BYTES", 0, 1)
    v, p = _run(gpu_device, i, kind)
    _compare(v, p, i, kind, what="bf16 planes, %s %s" % (kind, S.GIBBS_SHAPES[i]))
    if kind == "free":
        assert np.array_equal(_bits(v), _bits(free8[i][0])) and np.array_equal(_bits(p), _bits(free8[i][1]))


@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_chain0(gpu_device, i):
    v, p = _run(gpu_device, i, "free", chain0=8)
    _compare(v, p, i, "free", chain0=8, what="chain0 = 8 %s" % (S.GIBBS_SHAPES[i],))


def test_gibbs_run_labels_refusals(gpu_device):
    from keras_unsupervised_amd._lib import KurbmError
    params, v0, _, _, _ = S.gibbs_fixture(0, "free")
    e = _engine(*params, gpu_device)
    x = _wide(v0, gpu_device)
    for bad in (1, 65, 70, -3):
        with pytest.raises(KurbmError, match="n_labels"):
            e.gibbs_run(x, n_labels=bad)
    with pytest.raises(KurbmError, match="Bernoulli"):
        e.gibbs_run(x, n_labels=10, mode=1)
    with pytest.raises(KurbmError, match="multiple of 4"):
        e.gibbs_run(x, n_labels=10, chain0=2)
    short = torch.zeros(e.gibbs_workspace(37, 17, 0).numel() - 16, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(KurbmError, match="too small"):
        e.gibbs_run(x, n_labels=10, ws=short)


# ---- 2. AIS: one temperature, teacher-forced -----------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", S.AIS_BETAS)
@pytest.mark.parametrize("chain0", [0, 6])
@pytest.mark.parametrize("shape", S.AIS_SHAPES)
def test_ais_step_labels_against_restatement(gpu_device, shape, chain0, betas):
    rows, n_pix, C, n_hid = shape
    beta_prev, beta = betas
    k, seed = S.AIS_K, S.AIS_SEED
    W, b_h, b_v, b_a, v = S.ais_model(shape)
    e = _engine(W, b_h, b_v, gpu_device)
    out = _np(e.ais_step_labels(_wide(v, gpu_device), C, beta_prev, beta, k, base_bias=b_a, chain0=chain0, seed=seed))
    torch.cuda.synchronize()
    e.check_status()

    ph, uh, h_ref = A.hidden(W, b_h, beta, k, v, chain0, seed)
    assert np.array_equal(_bits(out["u_h"]), _bits(uh)), "hidden uniforms must be bit-exact"
    assert np.max(np.abs(out["prob_h"] - ph)) <= TOL
    assert np.array_equal(out["h"], (out["u_h"] < out["prob_h"]).astype(np.float32))
    assert np.all(np.abs(uh - ph)[out["h"] != h_ref] <= FLIP_BAND)

    # v_out is drawn from the GPU's own h: the restatement is fed that h
    pv, u, py, v_ref, _ = S.ais_visible(W, b_v, b_a, beta, k, out["h"], n_pix, chain0, seed)
    assert np.array_equal(_bits(out["u_v"][:, :n_pix]), _bits(u[:, :n_pix])), "pixel uniforms must be bit-exact"
    assert np.array_equal(_bits(out["u_y"]), _bits(u[:, n_pix])), "the label uniform must be bit-exact"
    assert np.max(np.abs(out["prob_v"][:, :n_pix] - pv)) <= TOL and np.max(np.abs(out["prob_y"] - py)) <= TOL
    vg = out["v"]
    assert np.array_equal(vg[:, :n_pix], (out["u_v"][:, :n_pix] < out["prob_v"][:, :n_pix]).astype(np.float32))
    # the class is that of the GPU's own p and u: the first c whose running fp32 sum exceeds u, else C - 1
    cum = np.cumsum(out["prob_y"], axis=1, dtype=np.float32)
    below = out["u_y"][:, None] < cum
    cls = np.where(below.any(axis=1), below.argmax(axis=1), C - 1)
    assert np.array_equal(vg[:, n_pix:], L.one_hot(cls, C)), "the block must be the draw of the GPU's own p and u"
    differ = vg[:, :n_pix] != v_ref[:, :n_pix]
    assert np.all(np.abs(u[:, :n_pix].astype(np.float64) - pv)[differ] <= FLIP_BAND)
    margin = L.draw_class(py, u[:, n_pix])[1]
    assert np.all(margin[(vg[:, n_pix:] != v_ref[:, n_pix:]).any(axis=1)] <= FLIP_BAND), "a class differs outside the band"

    d_ref, mag = S.ais_delta(W, b_h, b_v, b_a, beta_prev, beta, v)
    err = np.abs(out["dlogw"].astype(np.float64) - d_ref)
    print("max |Delta_gpu - Delta_ref| / max(1, magnitude) = %.3g" % np.max(err / np.maximum(1.0, mag)))
    assert np.all(err <= TOL * np.maximum(1.0, mag))


@pytest.mark.parametrize("shape", S.AIS_SHAPES)
def test_ais_run_labels_is_the_loop_of_step_hooks(gpu_device, shape):
    """A short run equals the loop of step hooks fed its own states, from the start the restatement states: the states bit for bit;
    logw against the hooks' Delta_k summed in double.  The two add the same fp32 terms of (b_v - b_A).v in another order (the run
    keeps them per group of 16 columns, the hook's start launch as one sum per chain -- as kurbm_ais_run and kurbm_ais_step do), so
    each temperature may differ by fp32 rounding of that sum: the step test's bar, TOL max(1, magnitude), summed over the
    temperatures.  And the run is reproducible."""
    rows, n_pix, C, n_hid = shape
    W, b_h, b_v, b_a, _ = S.ais_model(shape)
    chain0, seed = 4, S.AIS_SEED
    e = _engine(W, b_h, b_v, gpu_device)
    logw, vf = e.ais_run(S.RUN_BETAS, rows, base_bias=b_a, chain0=chain0, seed=seed, want_v=True, n_labels=C)
    logw2, vf2 = e.ais_run(S.RUN_BETAS, rows, base_bias=b_a, chain0=chain0, seed=seed, want_v=True, n_labels=C)
    torch.cuda.synchronize()
    logw, vf = logw.cpu().numpy(), vf.to_numpy()
    assert np.array_equal(logw.view(np.uint64), logw2.cpu().numpy().view(np.uint64)) and np.array_equal(vf, vf2.to_numpy())
    v0, near = S.ais_start(b_a, n_pix, rows, chain0, seed)
    ok = ~near          # (a start draw inside the band may legitimately differ on the GPU: those chains prove nothing here)
    assert ok.sum() >= 0.9 * rows
    v, acc, bar = v0.astype(np.float32), np.zeros(rows), np.zeros(rows)
    for k in range(1, S.RUN_BETAS.size):
        bar += TOL * np.maximum(1.0, S.ais_delta(W, b_h, b_v, b_a, S.RUN_BETAS[k - 1], S.RUN_BETAS[k], v)[1])
        out = _np(e.ais_step_labels(_wide(v, gpu_device), C, S.RUN_BETAS[k - 1], S.RUN_BETAS[k], k, base_bias=b_a, chain0=chain0,
                                    seed=seed, want_planes=False))
        acc += out["dlogw"].astype(np.float64)
        v = out["v"]
    assert np.array_equal(vf[ok], v[ok]), "v_final must be the last hook's state"
    print("max |logw - sum of the hooks' Delta_k| = %.3g (bar %.3g)" % (np.max(np.abs(logw - acc)[ok]), bar.min()))
    assert np.all(np.abs(logw - acc)[ok] <= bar[ok]), "logw must be the hooks' Delta_k summed in double, up to the order of fp32 additions"
    logw_ref, _, flagged = S.ais_run(W, b_h, b_v, b_a, C, S.RUN_BETAS, rows, chain0, seed)
    ok = ~flagged
    assert flagged.sum() <= 0.10 * rows and np.max(np.abs(logw[ok] - logw_ref[ok]) / np.maximum(1.0, np.abs(logw_ref[ok]))) <= TOL


def test_ais_labels_refusals_and_the_size_query(gpu_device):
    from keras_unsupervised_amd._lib import KurbmError
    W, b_h, b_v, b_a, v = S.ais_model(S.AIS_SHAPES[0])
    e = _engine(W, b_h, b_v, gpu_device)
    for bad in (1, 65, 70):
        with pytest.raises(KurbmError, match="n_labels"):
            e.ais_run([0.0, 1.0], 8, base_bias=b_a, n_labels=bad, ws=torch.zeros(1 << 20, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(KurbmError, match="betas"):
        e.ais_run([0.0, 0.5], 8, base_bias=b_a, n_labels=10)
    short = torch.zeros(e.ais_workspace(8, 10).numel() - 16, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(KurbmError, match="workspace too small"):
        e.ais_run([0.0, 1.0], 8, base_bias=b_a, n_labels=10, ws=short)
    # n_pix = 33, C = 2: the site's group row is one more than the plain run's workspace holds
    q = lambda f, *a: int(f(e.ctx.handle, *a))
    assert q(e.lib.kurbm_ais_labels_workspace_bytes, 1024, 35, 8, 2) > q(e.lib.kurbm_ais_workspace_bytes, 1024, 35, 8)
    assert q(e.lib.kurbm_ais_labels_workspace_bytes, 8, 35, 8, 35) == 0 and q(e.lib.kurbm_ais_labels_workspace_bytes, 8, 35, 8, 1) == 0


def test_ais_run_labels_at_the_extra_group_row(gpu_device):
    """n_pix = 33, C = 2: ceil(33 / 16) + 1 = 4 group rows where ceil(35 / 16) = 3; the run against the restatement."""
    shape = (40, 33, 2, 20)
    W, b_h, b_v, b_a, _ = S.ais_model(shape)
    e = _engine(W, b_h, b_v, gpu_device)
    logw, vf = e.ais_run(S.RUN_BETAS, 40, base_bias=b_a, chain0=0, seed=3, want_v=True, n_labels=2)
    logw_ref, v_ref, flagged = S.ais_run(W, b_h, b_v, b_a, 2, S.RUN_BETAS, 40, 0, 3)
    ok = ~flagged
    logw = logw.cpu().numpy()
    assert flagged.sum() <= 4 and np.array_equal(vf.to_numpy()[ok], v_ref[ok].astype(np.float32))
    assert np.max(np.abs(logw[ok] - logw_ref[ok]) / np.maximum(1.0, np.abs(logw_ref[ok]))) <= TOL


# ---- 3. the estimate and the public calls on enumerable models ------------------------------------------------------------------
def _rbm(W, b_h, b_v, C, device, seed=5):
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM
    r = RBM(HPS, W.shape[1], mode=MODE_VISIBLE_BERNOULLI, seed=seed, weights=(W, b_h, b_v), device=device, n_labels=C)
    r.build((None, W.shape[0]))
    return r


def test_log_partition_with_labels_against_exact(gpu_device):
    """10 pixels, 3 classes, 9 hidden units, 256 chains, 400 temperatures: |z_gpu - exact| <= 5 se_ref, the existing rule."""
    from keras_unsupervised_amd.ebm import ais
    W, b_h, b_v, b_a = S.est_model()
    n_pix, C, n_hid = S.EST
    exact = ais.exact_log_partition(W, b_h, b_v, n_labels=C)
    z_ref, se_ref, _ = S.est_run()
    assert abs(z_ref - exact) <= 3.0 * se_ref
    rbm = _rbm(W, b_h, b_v, C, gpu_device, seed=S.EST_SEED)
    z_gpu = rbm.log_partition(n_chains=S.EST_CHAINS, betas=S.EST_TEMPS, base_rates=b_a, label="free")
    print("exact %.6f, gpu %.6f (error %+.4f), restatement error %+.4f, SE_ref %.4f, SE_gpu %.4f"
          % (exact, z_gpu, z_gpu - exact, z_ref - exact, se_ref, rbm.last_ais["stderr"]))
    assert abs(z_gpu - exact) <= 5.0 * se_ref
    assert rbm.last_ais["n_chains"] == S.EST_CHAINS and rbm.last_ais["n_betas"] == S.EST_TEMPS + 1
    assert abs(rbm.last_ais["log_z0"] - S.ais_log_z0(b_a, n_hid, n_pix)) <= 1e-9
    assert abs(rbm.log_partition(method="exact", label="free") - exact) <= 1e-9

    # log_likelihood, joint and marginal, with log_z given
    g = np.random.default_rng(4)
    V = (g.random((50, n_pix)) < .5).astype(np.float32)
    y = g.integers(0, C, 50)
    joined = np.concatenate([V, L.one_hot(y, C)], axis=1)
    ref_joint = float(S.log_joint(W, b_h, b_v, joined, exact).mean())
    ref_marg = float(S.log_marginal(W, b_h, b_v, V, n_pix, exact).mean())
    for got, ref in ((rbm.log_likelihood(V, y=y, log_z=exact, label="free"), ref_joint),
                     (rbm.log_likelihood(joined, log_z=exact, label="free"), ref_joint),
                     (rbm.log_likelihood(V, log_z=exact, label="free"), ref_marg)):
        print("log likelihood %.6f, restatement %.6f" % (got, ref))
        assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref))
    assert ref_marg > ref_joint


@pytest.fixture(scope="module")
def dist_rbm(gpu_device):
    W, b_h, b_v = S.dist_model()
    return _rbm(W, b_h, b_v, S.DIST[1], gpu_device)


def test_sample_free_frequencies(gpu_device, dist_rbm):
    """RBM.sample(label='free') on the 192-state model: 8192 chains, 100 sweeps, every state inside the 5 sigma band."""
    W, b_h, b_v = S.dist_model()
    n_pix, C, _ = S.DIST
    v = dist_rbm.sample(S.DIST_CHAINS, burn_in=S.DIST_BURN, label="free")
    assert v.shape == (S.DIST_CHAINS, n_pix + C) and set(np.unique(v)) <= {0.0, 1.0}
    assert np.array_equal(v[:, n_pix:].sum(axis=1), np.ones(S.DIST_CHAINS))
    p = S.exact_joint(W, b_h, b_v, n_pix)
    bad, f = S.joint_band_violations(v, p, n_pix, 5.0)
    print("max |f - p| = %.4f over %d states" % (np.max(np.abs(f - p)), p.size))
    assert bad.size == 0, (bad, f[bad], p[bad])


def test_gibbs_with_pixels_clamped_samples_the_posterior(gpu_device, dist_rbm):
    """gibbs(v, clamp = every pixel, label='free'): the class frequencies are predict_proba's."""
    n_pix, C, _ = S.DIST
    pix = np.tile(np.array([[1, 0, 1, 1, 0, 0]], np.float32), (4096, 1))
    post = dist_rbm.predict_proba(pix[:1])[0].astype(np.float64)
    v = dist_rbm.gibbs(pix, n_steps=3, clamp=list(range(n_pix)), label="free")
    assert np.array_equal(v[:, :n_pix], pix) and np.array_equal(v[:, n_pix:].sum(axis=1), np.ones(4096))
    f = v[:, n_pix:].mean(axis=0)
    print("class frequencies %s, posterior %s" % (np.round(f, 4), np.round(post, 4)))
    assert np.all(np.abs(f - post) <= 5.0 * np.sqrt(post * (1 - post) / 4096) + 1.0 / 4096)


def test_dbn_sample_free_returns_the_sampled_classes(gpu_device):
    from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, RBM
    g = np.random.default_rng(6)
    low = RBM(HPS, 6, mode=MODE_VISIBLE_BERNOULLI, seed=1, device=gpu_device,
              weights=(g.normal(0, .3, (12, 6)).astype(np.float32), np.zeros(6, np.float32), np.zeros(12, np.float32)))
    low.build((None, 12))
    W, b_h, b_v = S.dist_model()
    top = _rbm(W, b_h, b_v, S.DIST[1], gpu_device)
    dbn = DBN()
    dbn.add_stack(low)
    dbn.add_stack(top)
    out, y = dbn.sample(2048, burn_in=50, label="free", return_labels=True)
    assert out.shape == (2048, 12) and set(np.unique(out)) <= {0.0, 1.0} and y.shape == (2048,) and y.dtype.kind == "i"
    py = S.exact_joint(W, b_h, b_v, S.DIST[0]).reshape(S.DIST[1], -1).sum(axis=1)
    f = np.bincount(y, minlength=S.DIST[1]) / 2048.0
    assert np.all(np.abs(f - py) <= 5.0 * np.sqrt(py * (1 - py) / 2048) + 1.0 / 2048)
