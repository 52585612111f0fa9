"""CPU tier of the softmax label units: the yardstick of tests/test_gpu_labels.py -- the float64 restatement of tests/labels_ref.py
must give the enumerated p(y | v) of a small model and draw its classes with the stated frequencies -- the C ABI's new symbols,
the host-side argument checks of RBM(n_labels=...), and the properties the GPU tier's fixtures rest on (no draw of a fixture
inside the band where an fp32 kernel may legitimately decide the other way), so that no fixture can silently rot."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # labels_ref.py lives beside this file
import labels_ref as R
from keras_unsupervised_amd import _lib
from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, RBM
from keras_unsupervised_amd.ebm.engine import DeviceMatrix

HPS = {"batch_size": 4, "epochs": 1, "lr": 0.1}
NEW_SYMBOLS = ("kurbm_label_sample", "kurbm_cd_step_labels", "kurbm_cd_epoch_labels", "kurbm_class_workspace_bytes", "kurbm_class_logits")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_posterior_equals_enumeration():
    """6 pixels, 3 classes, 5 hidden units: softmax of the restated class logits is the joint summed over all 32 hidden states."""
    W, b_h, b_v = R.model(6, 3, 5)
    v = (np.random.default_rng(1).random((16, 6)) < .5).astype(np.float32)
    logits, mag = R.class_logits(W, b_h, b_v, v, 6)
    p = R.posterior(logits)
    assert p.shape == (16, 3) and np.max(np.abs(p.sum(axis=1) - 1.0)) <= 1e-12
    assert np.max(np.abs(p - R.exact_posterior(W, b_h, b_v, v, 6))) <= 1e-12
    assert np.all(mag >= np.abs(logits))
    # F(v, y = c) differs from -logit_c by the class-independent pixel term only, and a label block behind the pixels is ignored
    F = R.joint_free_energy(W, b_h, b_v, v, 6)
    assert np.max(np.abs((F + logits) - (F + logits)[:, :1])) <= 1e-12
    wide = np.concatenate([v, R.one_hot(np.arange(16) % 3, 3)], axis=1)
    assert np.array_equal(R.class_logits(W, b_h, b_v, wide, 6)[0], logits)


def test_label_site_frequencies():
    """20 000 restated draws of one hidden state: the class counts match p (chi-square, p > 1e-3, fixed seed)."""
    n, n_pix, C, n_hid = 20000, 6, 5, 8
    W, _, b_v = R.model(n_pix, C, n_hid, seed=3, std=.8)
    h = np.tile((np.random.default_rng(4).random(n_hid) < .5).astype(np.float32), (n, 1))
    p, u, cls, _ = R.label_site(W, b_v, h, n_pix, 12345, 9, 0)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0 and np.max(np.abs(p - p[0])) == 0.0
    counts = np.bincount(cls, minlength=C)
    chi2 = float((((counts - n * p[0]) ** 2) / (n * p[0])).sum())
    pval = R.chi2_sf(chi2, C - 1)
    print("counts %s, expected %s, chi2 %.3f, p %.4f" % (counts, np.round(n * p[0], 1), chi2, pval))
    assert counts.min() > 0 and pval > 1e-3


def test_draw_rule_and_chi2_helper():
    p = np.array([[.2, .3, .5], [.2, .3, .5], [.2, .3, .5], [1.0, 0.0, 0.0], [.3, .3, .3]])
    cls, margin = R.draw_class(p, np.array([.1, .2, .999, .5, .95], np.float32))
    assert cls.tolist() == [0, 1, 2, 0, 2]          # u = p_0 exactly goes to the next class; nothing below a boundary -> C - 1
    assert abs(margin[0] - .1) < 1e-7 and margin[1] < 1e-7
    assert abs(R.chi2_sf(3.0, 2) - np.exp(-1.5)) < 1e-12 and abs(R.chi2_sf(20.0, 9) - 0.017912) < 1e-5 and R.chi2_sf(0.0, 4) == 1.0
    assert np.array_equal(R.one_hot([2, 0], 3), np.array([[0, 0, 1], [1, 0, 0]], np.float32))


# ---- the fixtures of the GPU tier ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SITE_SHAPES + R.LOOP_SHAPES)
def test_site_fixtures_stay_clear_of_the_boundaries(shape):
    rows, n_pix, C, n_hid = shape
    W, b_v, h = R.site_inputs(*shape)
    assert W.shape == (n_pix + C, n_hid) and h.shape == (rows, n_hid)
    _, _, cls, margin = R.label_site(W, b_v, h, n_pix, R.SITE_SEED, R.SITE_STREAM, R.SITE_STEP)
    print("%s: nearest |u - boundary| = %.3g" % (shape, margin.min()))
    assert margin.min() > R.FLIP_BAND and cls.min() >= 0 and cls.max() < C
    assert len(set(cls.tolist())) >= 3, "a fixture whose rows all draw one class would not notice a wrong sum"


def test_first_site_fixture_margin_is_the_issues():
    W, b_v, h = R.site_inputs(*R.SITE_SHAPES[0])
    _, _, _, margin = R.label_site(W, b_v, h, 37, R.SITE_SEED, R.SITE_STREAM, R.SITE_STEP)
    assert abs(margin.min() - 1.8e-4) < 1e-5


def test_anchored_step_and_trajectory_have_no_draw_in_the_band():
    rows, n_pix, C, n_hid = R.ANCHOR
    W, b_h, b_v = R.model(n_pix, C, n_hid)
    V, _ = R.labelled_batch(rows, n_pix, C)
    s = R.cd_step(W, b_h, b_v, V, C, R.ANCHOR_SEED, R.ANCHOR_STEP)
    assert s["margin"] > R.FLIP_BAND
    assert np.array_equal(s["v_neg"][:, n_pix:].sum(axis=1), np.ones(rows)) and set(np.unique(s["v_neg"])) <= {0.0, 1.0}
    assert np.array_equal(s["db_v"][n_pix:], np.round(s["db_v"][n_pix:])) and s["db_v"][n_pix:].sum() == 0.0
    N, n_pix, C, n_hid = R.FIT_SHAPE
    W, b_h, b_v = R.model(n_pix, C, n_hid, std=.1)
    V, _ = R.labelled_batch(N, n_pix, C)
    out = R.fit(W, b_h, b_v, V, C, R.FIT_BATCH, 1, R.FIT_LR, R.FIT_SEED)
    assert out[3] == 3 and out[4] > R.FLIP_BAND


def test_restatement_learns_the_prototypes():
    L = R.LEARN
    X, y = R.prototypes_data()
    W, b_h, b_v = R.learn_init()
    out = R.fit(W, b_h, b_v, np.concatenate([X, R.one_hot(y, L["C"])], axis=1), L["C"], L["batch"], L["epochs"], L["lr"], L["seed"])
    acc = float((R.predict(out[0], out[1], out[2], X, L["n_pix"]) == y).mean())
    print("restatement accuracy %.4f" % acc)
    assert acc >= 2.0 / L["C"]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kurbm.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define KURBM_ABI_VERSION 5" in text and lib.kurbm_abi_version() == 5
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [13, 12, 12, 4, 12]
    # a null context is refused before anything else is looked at
    assert lib.kurbm_class_workspace_bytes(None, 8, 8, 8) == 0
    assert lib.kurbm_label_sample(None, None, 3, None, 8, 8, None, None, 8, None, 0, None, None) == -1
    assert lib.kurbm_cd_step_labels(None, None, 3, None, 8, 8, None, 7, None, 0, None, None) == -1
    assert lib.kurbm_cd_epoch_labels(None, None, 3, None, 8, 8, 4, None, None, 0, None, None) == -1
    assert lib.kurbm_class_logits(None, None, 3, None, 8, 8, None, 4, None, None, 0, None) == -1


# ---- host logic --------------------------------------------------------------------------------------------------------------
class FakeEngine:
    def __init__(self, n_vis, n_hid):
        self.n_vis, self.n_hid, self.device = n_vis, n_hid, torch.device("cpu")
        self.b_v = torch.zeros(n_vis)
        self.calls = []

    def philox_uniform(self, rows, cols, seed, stream_id, step, row0=0):
        m = DeviceMatrix.zeros(rows, cols, self.device)
        m.view().fill_(0.25)
        return m

    def gibbs_run(self, v, burn_in=1, thin=1, n_keep=1, chain0=0, seed=0, mode=0, clamp=None, want_prob=False, ws=None):
        self.calls.append(("gibbs", v.view().clone(), None if clamp is None else np.asarray(clamp).copy()))
        out = DeviceMatrix.zeros(n_keep * v.rows, self.n_vis, self.device)
        out.t[:, : self.n_vis] = v.view().repeat(n_keep, 1)
        return out, None

    def class_logits(self, v, n_labels, rows=None, row_start=0, want_prob=True, ws=None):
        self.calls.append(("class_logits", v.rows, v.cols, n_labels))
        lg = DeviceMatrix.zeros(v.rows, n_labels, self.device)
        lg.t[:, 1] = 1.0
        pr = DeviceMatrix.zeros(v.rows, n_labels, self.device)
        pr.view().copy_(torch.softmax(lg.view(), dim=1))
        return lg, pr


def fake_rbm(n_pix=6, C=3, n_hid=4):
    r = RBM(HPS, n_hid, mode=MODE_VISIBLE_BERNOULLI, seed=11, n_labels=C)
    r._dev = FakeEngine(n_pix + C, n_hid)
    r.input_shape, r.output_shape, r.built = (None, n_pix + C), (None, n_hid), True
    return r


def test_constructor_arguments():
    for bad in (1, 65, -2):
        with pytest.raises(ValueError, match="n_labels"):
            RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=bad)
    with pytest.raises(ValueError, match="MODE_VISIBLE_BERNOULLI"):
        RBM(HPS, 4, mode=MODE_VISIBLE_GAUSSIAN, n_labels=3)
    with pytest.raises(ValueError, match="MODE_VISIBLE_BERNOULLI"):
        RBM(HPS, 4, n_labels=3)                                  # (the reference's default mode is the Gaussian one)
    assert RBM(dict(HPS, n_labels=5), 4, mode=MODE_VISIBLE_BERNOULLI).n_labels == 5          # an hps key works too
    assert RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI).n_labels == 0
    r = RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3)
    with pytest.raises(ValueError, match="no pixel"):
        r.build((None, 3))
    # whatever path was asked for, a label RBM trains on the five-launch fp32 one
    for c in ("auto", "x3", "small", "bf16", "fp32"):
        assert RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3, compute_dtype=c)._compute() == "fp32"
    assert RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, compute_dtype="x3")._compute() == "x3"


def test_config_round_trip():
    r = RBM(HPS, 7, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=3, n_labels=10, momentum=0.5)
    cfg = r.get_config()
    assert cfg["n_labels"] == 10
    r2 = RBM(**cfg)
    assert r2.n_labels == 10 and r2.get_config() == cfg
    assert RBM(HPS, 7, mode=MODE_VISIBLE_BERNOULLI).get_config()["n_labels"] == 0


def test_join():
    r = RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3)
    V = np.arange(8, dtype=np.float32).reshape(2, 4)
    J = r.join(V, [2, 0])
    assert J.dtype == np.float32 and J.shape == (2, 7)
    assert np.array_equal(J[:, :4], V) and np.array_equal(J[:, 4:], [[0, 0, 1], [1, 0, 0]])
    assert np.array_equal(r.join(torch.from_numpy(V), torch.tensor([2, 0])), J)
    for bad in ([0, 3], [-1, 0], [0], [0.5, 1.0]):
        with pytest.raises(ValueError):
            r.join(V, bad)
    with pytest.raises(ValueError, match="label RBM"):
        RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI).join(V, [0, 1])


def test_sampling_needs_a_clamped_block_and_likelihoods_are_refused():
    r = fake_rbm()
    v = np.zeros((4, 9), np.float32)
    for call in (lambda: r.sample(4, burn_in=1), lambda: r.gibbs(v), lambda: r.gibbs(v, clamp=[6, 7]),
                 lambda: r.sample(4, burn_in=1, init=v, clamp=[0, 6])):
        with pytest.raises(ValueError, match="label block clamped"):
            call()
    for call in (lambda: r.log_partition(), lambda: r.log_likelihood(v)):
        with pytest.raises(ValueError, match="label RBM"):
            call()
    with pytest.raises(ValueError, match="labels must be integers"):
        r.sample(4, burn_in=1, label=3)
    with pytest.raises(ValueError, match="label= needs a label RBM"):
        plain = fake_rbm()
        plain.n_labels = 0
        plain.sample(4, burn_in=1, label=1)
    assert r._dev.calls == []
    # label=: the chains start from the one-hot block and the whole block is clamped
    out = r.sample(4, burn_in=1, label=2)
    _, init, clamp = r._dev.calls[-1]
    assert np.array_equal(init[:, 6:].numpy(), np.tile([0, 0, 1], (4, 1))) and clamp.tolist() == [False] * 6 + [True] * 3
    assert out.shape == (4, 9) and np.array_equal(out[:, 6:], np.tile([0, 0, 1], (4, 1)))
    r.gibbs(np.ones((3, 6), np.float32), label=[0, 1, 2], clamp=[0])
    _, init, clamp = r._dev.calls[-1]
    assert np.array_equal(init[:, 6:].numpy(), np.eye(3)) and bool((init[:, :6] == 1).all()) and clamp.tolist() == [True] + [False] * 5 + [True] * 3
    # a clamp that covers the block with an init that carries it is the caller's own way to the same run
    r.gibbs(r.join(np.ones((3, 6), np.float32), [1, 1, 1]), clamp=[6, 7, 8])
    assert np.array_equal(r._dev.calls[-1][1][:, 6:].numpy(), np.tile([0, 1, 0], (3, 1)))


def test_data_parallel_fit_of_a_label_rbm_is_refused(monkeypatch):
    from keras_unsupervised_amd.ebm import dp
    r = fake_rbm()
    monkeypatch.setattr(dp, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="no data-parallel fit"):
        r.fit(np.zeros((4, 6), np.float32), verbose=0, y=[0, 1, 2, 0])
    assert r._dev.calls == [] and r._update_count == 0


def test_predict_on_the_double_and_fit_refusals():
    r = fake_rbm()
    for cols in (6, 9):
        p = r.predict_proba(np.zeros((5, cols), np.float32))
        assert isinstance(p, np.ndarray) and p.shape == (5, 3) and np.allclose(p.sum(axis=1), 1.0)
        y = r.predict(torch.zeros(5, cols))
        assert isinstance(y, torch.Tensor) and y.tolist() == [1] * 5
        assert r.class_logits(np.zeros((5, cols), np.float32)).shape == (5, 3)
    with pytest.raises(ValueError, match="columns"):
        r.predict(np.zeros((5, 7), np.float32))
    with pytest.raises(ValueError, match="label RBM"):
        RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI).fit(np.zeros((4, 6), np.float32), verbose=0, y=[0, 1, 0, 1])
    # fit without y: the block must be one-hot; with y: V holds the pixels alone
    with pytest.raises(ValueError, match="one-hot"):
        r.fit(np.zeros((4, 9), np.float32), verbose=0)
    with pytest.raises(ValueError, match="pixels alone"):
        r.fit(np.zeros((4, 9), np.float32), verbose=0, y=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="labels must be integers"):
        r.fit(np.zeros((4, 6), np.float32), verbose=0, y=[0, 1, 2, 3])


def test_dbn_accepts_a_label_rbm_on_top_only():
    lower = RBM(HPS, 6, mode=MODE_VISIBLE_BERNOULLI)
    lower._dev, lower.input_shape, lower.output_shape, lower.built = FakeEngine(8, 6), (None, 8), (None, 6), True
    dbn = DBN()
    dbn.add_stack(lower)
    dbn.add_stack(fake_rbm(n_pix=6))                      # 6 pixels + 3 labels on a layer of 6 hidden units
    with pytest.raises(ValueError, match="top of a DBN"):
        dbn.add_stack(RBM(HPS, 3, mode=MODE_VISIBLE_BERNOULLI))
    bad = DBN()
    bad.add_stack(lower)
    with pytest.raises(ValueError, match="output dimension"):
        bad.add_stack(fake_rbm(n_pix=5))
    with pytest.raises(ValueError, match="y goes with a label RBM"):
        dbn.fit(np.zeros((4, 8), np.float32), verbose=0)
    with pytest.raises(ValueError, match="label RBM"):
        bad.predict(np.zeros((4, 8), np.float32))
