"""CPU tier of the free label blocks: the yardstick of tests/test_gpu_labelsite.py -- the float64 restatement of
tests/labelsite_ref.py must sample the enumerated joint p(v, y) of a small label RBM and estimate its log Z -- the label-aware host
helpers of ebm/ais.py, the opt-in / refusal matrix of label='free' on a fake engine, the C ABI's new symbols, and the property the
GPU tier's fixtures rest on: the restatement alone flags at most 10 % of the chains of every fixture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # the *_ref.py modules live beside this file
import ais_ref as A
import gibbs_ref as G
import labels_ref as L
import labelsite_ref as S
from keras_unsupervised_amd import _lib
from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, RBM, ais
from keras_unsupervised_amd.ebm.engine import DeviceMatrix

HPS = {"batch_size": 4, "epochs": 1, "lr": 0.1}
NEW_SYMBOLS = ("kurbm_gibbs_run_labels", "kurbm_ais_labels_workspace_bytes", "kurbm_ais_run_labels", "kurbm_ais_step_labels")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamped", [False, True])
def test_restated_gibbs_chain_samples_the_enumerated_joint(clamped):
    """6 pixels, 3 classes, 5 hidden units: 8192 restated chains after 100 sweeps against p(v, y) over the 192 states (free), and
    against p(v, y | two clamped pixels); every state's frequency inside the 5 sigma band of the Gibbs tests."""
    W, b_h, b_v = S.dist_model()
    n_pix, C, _ = S.DIST
    v0, v = S.dist_run(clamped)
    assert set(np.unique(v)) <= {0.0, 1.0} and np.array_equal(v[:, n_pix:].sum(axis=1), np.ones(v.shape[0]))
    p = S.exact_joint(W, b_h, b_v, n_pix, S.DIST_CLAMP if clamped else None, S.DIST_VALUES if clamped else None)
    assert p.size == 192 and abs(p.sum() - 1.0) < 1e-12
    bad, f = S.joint_band_violations(v, p, n_pix, 5.0)
    print("clamped %s: max |f - p| = %.4f over %d states" % (clamped, np.max(np.abs(f - p)), p.size))
    assert bad.size == 0, (bad, f[bad], p[bad])
    if clamped:
        assert np.array_equal(v[:, S.DIST_CLAMP], v0[:, S.DIST_CLAMP])
    # the class frequencies are those of the marginal p(y): the block is sampled, not kept
    py = p.reshape(C, -1).sum(axis=1)
    fy = v[:, n_pix:].mean(axis=0)
    assert np.max(np.abs(fy - py)) <= 5.0 * np.sqrt(.25 / v.shape[0])


def test_restated_ais_estimate_against_label_aware_enumeration():
    """10 pixels, 3 classes, 9 hidden units: |z_ref - exact| <= 3 se_ref, the rule tests/test_ais_host.py holds its restatement to."""
    W, b_h, b_v, b_a = S.est_model()
    z, se, logw = S.est_run()
    exact = ais.exact_log_partition(W, b_h, b_v, n_labels=S.EST[1])
    print("restated log Z %.5f +- %.5f, exact %.5f" % (z, se, exact))
    assert np.isfinite(logw).all() and se > 0 and abs(z - exact) <= 3.0 * se


@pytest.mark.parametrize("shape", [(6, 3, 5), (4, 3, 7), (5, 2, 5)])
def test_exact_log_partition_with_labels_against_brute_force(shape):
    """Both enumerations (hidden side: n_hid <= n_pix; pixels x classes: n_hid > n_pix) against the loop over every (v, y, h)."""
    n_pix, C, n_hid = shape
    W, b_h, b_v = L.model(n_pix, C, n_hid, seed=40 + n_hid, std=.7)
    z = ais.exact_log_partition(W, b_h, b_v, n_labels=C)
    assert abs(z - S.brute_force_log_z(W, b_h, b_v, n_pix)) <= 1e-9
    # the label-blind sum counts the non-one-hot blocks too: a different, larger number
    assert ais.exact_log_partition(W, b_h, b_v) > z
    with pytest.raises(ValueError, match="n_labels"):
        ais.exact_log_partition(W, b_h, b_v, n_labels=n_pix + C)
    with pytest.raises(ValueError, match="n_labels"):
        ais.exact_log_partition(W, b_h, b_v, n_labels=1)


def test_joint_minus_marginal_is_the_posterior():
    W, b_h, b_v = S.dist_model()
    n_pix, C, _ = S.DIST
    v = (np.random.default_rng(2).random((16, n_pix)) < .5).astype(np.float32)
    log_z = ais.exact_log_partition(W, b_h, b_v, n_labels=C)
    marg = S.log_marginal(W, b_h, b_v, v, n_pix, log_z)
    post = L.posterior(L.class_logits(W, b_h, b_v, v, n_pix)[0])
    for c in range(C):
        joint = S.log_joint(W, b_h, b_v, np.concatenate([v, L.one_hot(np.full(16, c), C)], axis=1), log_z)
        assert np.max(np.abs((joint - marg) - np.log(post[:, c]))) <= 1e-12
    # and the marginal is normalised over the 64 pixel states
    allv = G.state_matrix(n_pix)
    assert abs(np.exp(S.log_marginal(W, b_h, b_v, allv, n_pix, log_z)).sum() - 1.0) <= 1e-12


def test_base_rate_bias_and_log_z0_with_labels():
    g = np.random.default_rng(3)
    n_pix, C = 5, 4
    y = g.integers(0, 3, 50)                      # class 3 never occurs: its entry stays finite
    V = np.concatenate([(g.random((50, n_pix)) < .3).astype(np.float64), L.one_hot(y, C)], axis=1)
    b = ais.base_rate_bias(V, n_labels=C)
    assert np.array_equal(b[:n_pix], ais.base_rate_bias(V)[:n_pix]) and np.isfinite(b).all()
    freq = np.bincount(y, minlength=C) / 50.0
    assert np.max(np.abs(b[n_pix:] - np.log(.95 * freq + .05 / C))) <= 1e-15
    assert abs(np.exp(b[n_pix:]).sum() - 1.0) <= 1e-12                  # a categorical base model: logsumexp = 0
    z0 = ais.log_z0(b, 7, n_labels=C)
    assert abs(z0 - (7 * np.log(2.0) + np.logaddexp(0.0, b[:n_pix]).sum())) <= 1e-12
    assert abs(z0 - S.ais_log_z0(b, 7, n_pix)) <= 1e-12
    # W = 0: the base model's log Z by enumeration
    assert abs(ais.exact_log_partition(np.zeros((n_pix + C, 7)), np.zeros(7), b, n_labels=C) - z0) <= 1e-9
    logw = g.normal(0, .1, 64)
    est = ais.estimate(logw, b, 7, n_labels=C)
    assert est[2] == z0 and abs(est[0] - (z0 + ais.log_mean_exp(logw))) <= 1e-12
    assert ais.log_z0(b, 7) != z0 and ais.estimate(logw, b, 7)[2] == ais.log_z0(b, 7)       # (the plain forms are unchanged)
    with pytest.raises(ValueError, match="n_labels"):
        ais.base_rate_bias(V, n_labels=n_pix + C)


# ---- the fixtures of the GPU tier: the restatement alone flags at most 10 % ---------------------------------------------------
@pytest.mark.parametrize("i", range(len(S.GIBBS_SHAPES)))
def test_gibbs_fixtures_flag_at_most_a_tenth(i):
    rows, n_pix, C, n_hid = S.GIBBS_SHAPES[i]
    assert S.KEEP["burn_in"] + (S.KEEP["n_keep"] - 1) * S.KEEP["thin"] <= 8
    for kind, chain0 in (("free", 0), ("free", 8), ("keep", 0), ("clamp", 0), ("real", 0)):
        _, v0, clamp, kw, (v, p, flagged) = S.gibbs_fixture(i, kind, chain0)
        print("%s %s chain0 %d: %d of %d flagged" % (S.GIBBS_SHAPES[i], kind, chain0, flagged.sum(), rows))
        assert flagged.sum() <= S.FLAG_CAP * rows
        assert np.array_equal(v[:, :, n_pix:].sum(axis=2), np.ones(v.shape[:2])) and set(np.unique(v[:, :, n_pix:])) <= {0.0, 1.0}
        assert np.max(np.abs(p[:, :, n_pix:].sum(axis=2) - 1.0)) <= 1e-12
        assert len(set(v[-1][:, n_pix:].argmax(axis=1).tolist())) >= 3, "a fixture whose chains all draw one class notices nothing"
        if clamp is not None:
            assert clamp.max() < n_pix and np.array_equal(v[-1][:, clamp], v0[:, clamp].astype(np.float64))
    # the clamped pixels share an 8-byte group of the plane with the block
    assert (S.gibbs_clamp(S.GIBBS_SHAPES[i]) // 8 == n_pix // 8).any() or n_pix % 8 == 0


@pytest.mark.parametrize("shape", S.AIS_SHAPES)
def test_ais_fixtures_flag_at_most_a_tenth(shape):
    rows, n_pix, C, n_hid = shape
    W, b_h, b_v, b_a, v = S.ais_model(shape)
    for beta_prev, beta in S.AIS_BETAS:
        for chain0 in (0, 6):
            ph, uh, h = A.hidden(W, b_h, beta, S.AIS_K, v, chain0, S.AIS_SEED)
            _, _, _, _, near = S.ais_visible(W, b_v, b_a, beta, S.AIS_K, h, n_pix, chain0, S.AIS_SEED)
            near = near | (np.abs(uh - ph) <= S.FLIP_BAND).any(axis=1)
            assert near.sum() <= S.FLAG_CAP * rows
    _, vf, flagged = S.ais_run(W, b_h, b_v, b_a, C, S.RUN_BETAS, rows, 4, S.AIS_SEED)
    assert flagged.sum() <= S.FLAG_CAP * rows and np.array_equal(vf[:, n_pix:].sum(axis=1), np.ones(rows))


def test_start_block_follows_the_site_rule():
    b_v = np.concatenate([np.zeros(6), np.log([.2, .3, .5])]).astype(np.float32)
    cls = S.start_block(b_v, 6, 20000, 8, 11)
    f = np.bincount(cls, minlength=3) / 20000.0
    assert np.max(np.abs(f - [.2, .3, .5])) <= 5.0 * np.sqrt(.25 / 20000)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kurbm.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define KURBM_ABI_VERSION 5" in text and lib.kurbm_abi_version() == 5
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [23, 5, 15, 27]
    # each is its plain twin plus n_labels (the step hook: plus prob_y, ldp, u_y)
    assert len(_lib.SIGNATURES["kurbm_gibbs_run"][1]) == 22 and len(_lib.SIGNATURES["kurbm_ais_run"][1]) == 14
    assert len(_lib.SIGNATURES["kurbm_ais_step"][1]) == 23
    assert "have no softmax site yet" not in text
    # a null context is refused before anything else is looked at
    assert lib.kurbm_ais_labels_workspace_bytes(None, 8, 8, 8, 3) == 0
    assert lib.kurbm_gibbs_run_labels(None, None, 3, None, 0, None, 1, 8, 8, 0, 0, 0, 1, 1, 1, None, None, None, 8, 0, None, 0, None) == -1
    assert lib.kurbm_ais_run_labels(None, None, 3, None, None, 2, 8, 0, 0, None, None, 0, None, 0, None) == -1
    assert lib.kurbm_ais_step_labels(None, None, 3, None, 0.0, 1.0, 1, None, 8, 8, 0, 0, None, None, 8, None, 8, None, None, None,
                                     None, None, 0, None, None, 0, None) == -1


# ---- host logic: the opt-in and refusal matrix on a fake engine ---------------------------------------------------------------
class FakeEngine:
    def __init__(self, n_vis, n_hid):
        self.n_vis, self.n_hid, self.device = n_vis, n_hid, torch.device("cpu")
        self.b_v = torch.zeros(n_vis)
        self.calls = []

    def philox_uniform(self, rows, cols, seed, stream_id, step, row0=0):
        m = DeviceMatrix.zeros(rows, cols, self.device)
        m.view().fill_(0.5)
        return m

    def gibbs_run(self, v, burn_in=1, thin=1, n_keep=1, chain0=0, seed=0, mode=0, clamp=None, want_prob=False, ws=None, n_labels=0):
        self.calls.append(("gibbs", v.view().clone(), None if clamp is None else np.asarray(clamp).copy(), n_labels))
        out = DeviceMatrix.zeros(n_keep * v.rows, self.n_vis, self.device)
        out.t[:, : self.n_vis] = v.view().repeat(n_keep, 1)
        return out, None

    def ais_run(self, betas, n_chains, base_bias=None, chain0=0, seed=0, want_v=False, ws=None, n_labels=0):
        self.calls.append(("ais", int(np.asarray(betas).size), n_chains, np.asarray(base_bias).copy(), n_labels))
        return torch.zeros(n_chains, dtype=torch.float64), None

    def get_weights(self):
        return np.zeros((self.n_vis, self.n_hid), np.float32), np.zeros(self.n_hid, np.float32), np.zeros(self.n_vis, np.float32)

    def free_energy(self, v, rows, row_start=0, compute=None):
        self.calls.append(("free_energy", v.view().clone()))
        return torch.full((rows,), -2.0)

    def class_logits(self, v, n_labels, rows=None, row_start=0, want_prob=True, ws=None):
        self.calls.append(("class_logits", v.rows, v.cols, n_labels))
        return DeviceMatrix.zeros(v.rows, n_labels, self.device), None


def fake_rbm(n_pix=6, C=3, n_hid=4):
    r = RBM(HPS, n_hid, mode=MODE_VISIBLE_BERNOULLI, seed=11, n_labels=C)
    r._dev = FakeEngine(n_pix + C, n_hid)
    r.input_shape, r.output_shape, r.built = (None, n_pix + C), (None, n_hid), True
    return r


def test_refusals_point_at_the_opt_in():
    r = fake_rbm()
    v = np.zeros((4, 9), np.float32)
    for call in (lambda: r.sample(4, burn_in=1), lambda: r.gibbs(v)):
        with pytest.raises(ValueError, match=r"label block clamped.*label='free'"):
            call()
    for call in (lambda: r.log_partition(), lambda: r.log_likelihood(v)):
        with pytest.raises(ValueError, match=r"label RBM.*label='free'"):
            call()
    for call in (lambda: r.sample(4, burn_in=1, label="fre"), lambda: r.gibbs(v, label="Free"),
                 lambda: r.log_partition(label=2), lambda: r.log_likelihood(v, label="joint")):
        with pytest.raises(ValueError, match="free"):
            call()
    plain = fake_rbm()
    plain.n_labels = 0
    for call in (lambda: plain.sample(4, burn_in=1, label="free"), lambda: plain.gibbs(v, label="free"),
                 lambda: plain.log_partition(label="free"), lambda: plain.log_likelihood(v, label="free")):
        with pytest.raises(ValueError, match="label= needs a label RBM"):
            call()
    with pytest.raises(ValueError, match="y= needs"):
        plain.log_likelihood(v, y=[0, 1, 2, 0], log_z=0.0)
    assert r._dev.calls == [] and plain._dev.calls == []


def test_free_gibbs_and_sample_on_the_fake_engine():
    r = fake_rbm()
    # init=None: pixels [u < sigmoid(0)] (u = .5: off), the block one-hot from softmax(0, 0, 0) at u = .5: class 1
    out = r.sample(4, burn_in=1, label="free")
    _, init, clamp, n_labels = r._dev.calls[-1]
    assert n_labels == 3 and clamp is None and out.shape == (4, 9)
    assert np.array_equal(init[:, 6:].numpy(), np.tile([0, 1, 0], (4, 1))) and bool((init[:, :6] == 0).all())
    # pixels clamped: conditional (y, h | clamped pixels); the mask holds the pixels alone
    one_hot = r.join(np.ones((3, 6), np.float32), [2, 0, 1])
    r.gibbs(one_hot, clamp=[0, 5], label="free")
    _, init, clamp, n_labels = r._dev.calls[-1]
    assert n_labels == 3 and clamp.tolist() == [True] + [False] * 4 + [True] + [False] * 3 and np.array_equal(init.numpy(), one_hot)
    # "sample a class for this image": pixels alone, every pixel clamped
    r.gibbs(np.ones((3, 6), np.float32), clamp=list(range(6)), label="free")
    _, init, clamp, n_labels = r._dev.calls[-1]
    assert n_labels == 3 and init.shape == (3, 9) and clamp.tolist() == [True] * 6 + [False] * 3
    assert np.array_equal(init[:, 6:].sum(dim=1).numpy(), np.ones(3)) and bool((init[:, :6] == 1).all())
    # a clamp over the WHOLE block is today's clamped run; over part of it, refused
    n = len(r._dev.calls)
    r.gibbs(one_hot, clamp=[6, 7, 8], label="free")
    assert r._dev.calls[-1][3] == 0 and r._dev.calls[-1][2].tolist() == [False] * 6 + [True] * 3
    with pytest.raises(ValueError, match="part of the label block"):
        r.gibbs(one_hot, clamp=[0, 7], label="free")
    with pytest.raises(ValueError, match="part of the label block"):
        r.sample(3, burn_in=1, init=one_hot, clamp=[6, 7], label="free")
    # an init / v whose block is not one-hot is refused
    bad = one_hot.copy()
    bad[1, 6:] = [1, 1, 0]
    half = one_hot.copy()
    half[2, 6:] = [.5, .5, 0]
    for b in (bad, half, np.zeros((3, 9), np.float32)):
        with pytest.raises(ValueError, match="one-hot"):
            r.sample(3, burn_in=1, init=b, label="free")
        with pytest.raises(ValueError, match="one-hot"):
            r.gibbs(b, label="free")
    assert len(r._dev.calls) == n + 1
    # several kept samples per chain, and an init with the pixels alone
    out = r.sample(7, n_chains=3, burn_in=1, thin=1, init=np.ones((3, 6), np.float32), label="free")
    assert out.shape == (7, 9) and r._dev.calls[-1][3] == 3


def test_dbn_sample_passes_label_free_and_returns_labels():
    top = fake_rbm(n_pix=4, C=3)
    d = DBN.__new__(DBN)
    d._layers = lambda: [top]
    d._top_labels = lambda: 3
    out, y = d.sample(5, burn_in=1, label="free", return_labels=True)
    assert out.shape == (5, 7) and y.shape == (5,) and y.dtype.kind == "i" and np.array_equal(y, out[:, 4:].argmax(axis=1))
    assert top._dev.calls[-1][3] == 3
    out, y = d.sample(2, burn_in=1, label=[2, 0], return_labels=True)
    assert y.tolist() == [2, 0] and top._dev.calls[-1][3] == 0
    d._top_labels = lambda: 0
    with pytest.raises(ValueError, match="return_labels"):
        d.sample(2, burn_in=1, return_labels=True)


def test_log_partition_and_likelihood_on_the_fake_engine():
    r = fake_rbm()
    z = r.log_partition(n_chains=8, betas=5, label="free")
    kind, n_betas, n_chains, b_a, n_labels = r._dev.calls[-1]
    assert (kind, n_betas, n_chains, n_labels) == ("ais", 6, 8, 3) and not b_a.any()
    assert abs(z - (4 * np.log(2) + 6 * np.log(2) + np.log(3))) <= 1e-12 and r.last_ais["log_z0"] == z
    data = r.join((np.random.default_rng(0).random((10, 6)) < .5).astype(np.float32), np.arange(10) % 2)
    r.log_partition(n_chains=8, betas=5, base_rates=data, label="free")
    assert np.allclose(r._dev.calls[-1][3], ais.base_rate_bias(data, n_labels=3).astype(np.float32))
    assert abs(r.log_partition(method="exact", label="free") - (10 * np.log(2) + np.log(3))) <= 1e-9
    # joint: n_vis wide, or pixels with y=; marginal: pixels alone
    n = len(r._dev.calls)
    assert r.log_likelihood(data, log_z=1.0, label="free") == pytest.approx(2.0 - 1.0)
    assert r._dev.calls[-1][0] == "free_energy" and np.array_equal(r._dev.calls[-1][1].numpy(), data)
    assert r.log_likelihood(data[:, :6], y=np.arange(10) % 2, log_z=1.0, label="free") == pytest.approx(1.0)
    assert np.array_equal(r._dev.calls[-1][1].numpy(), data)
    assert r.log_likelihood(np.ones((2, 6), np.float32), log_z=1.0, label="free") == pytest.approx(np.log(3) - 1.0)
    assert r._dev.calls[-1] == ("class_logits", 2, 6, 3) and len(r._dev.calls) == n + 3
    # validated before any log Z is computed
    r.last_ais = None
    bad = data.copy()
    bad[0, 6:] = 1
    for call in (lambda: r.log_likelihood(bad, label="free"), lambda: r.log_likelihood(np.zeros((2, 5), np.float32), label="free"),
                 lambda: r.log_likelihood(data, y=np.zeros(10, np.int64), label="free"),
                 lambda: r.log_likelihood(data[:, :6], y=[3] * 10, label="free")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="label RBM"):
        r.log_likelihood(bad, label="free")
    assert len(r._dev.calls) == n + 3
    # without log_z the label-aware partition function is run (or its cached value used)
    r.log_likelihood(data, label="free", n_chains=4, betas=3)
    assert [c[0] for c in r._dev.calls[n + 3:]] == ["ais", "free_energy"] and r._dev.calls[n + 3][4] == 3
