"""CPU tier of discriminative / hybrid training: the yardstick of tests/test_gpu_classgrad.py -- the float64 restatement of
tests/classgrad_ref.py must agree with central differences of sum log p(y | v) and must learn the prototype classes -- the C
ABI's new symbols, and the host logic of RBM(objective=...) on an engine double: validation, the epoch path against the step path,
the update counter, the config and checkpoint keys.  A call the host refuses reaches no engine call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # labels_ref.py and classgrad_ref.py live beside this file
import classgrad_ref as G
import labels_ref as R
from keras_unsupervised_amd import _lib
from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM
from keras_unsupervised_amd.ebm.engine import DeviceMatrix

HPS = {"batch_size": 4, "epochs": 2, "lr": 0.1}
NEW_SYMBOLS = ("kurbm_disc_workspace_bytes", "kurbm_class_grad", "kurbm_disc_step", "kurbm_disc_epoch")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_gradient_equals_central_differences():
    n_pix, C, n_hid, rows, eps = 7, 3, 5, 9, 1e-5
    W, b_h, b_v = [x.astype(np.float64) for x in R.model(n_pix, C, n_hid)]
    V, _ = R.labelled_batch(rows, n_pix, C)
    out = G.class_grad(W, b_h, b_v, V, C)
    total = lambda *prm: -G.class_grad(*prm, V, C)["nll"].sum()
    worst = 0.0
    for which, (x, grad) in enumerate(((W, out["dW"]), (b_h, out["db_h"]), (b_v, out["db_v"]))):
        for idx in np.ndindex(x.shape):
            prm = [W.copy(), b_h.copy(), b_v.copy()]
            prm[which][idx] += eps
            up = total(*prm)
            prm[which][idx] -= 2 * eps
            num = (up - total(*prm)) / (2 * eps)
            dev = abs(num - grad[idx]) / max(1.0, abs(grad[idx]))
            worst = max(worst, dev)
            assert dev <= 1e-6, (which, idx, num, grad[idx])
    print("worst deviation from central differences %.3g" % worst)
    # the pieces are consistent with one another
    assert np.allclose(out["g"], out["S_y"] - out["H_bar"], atol=1e-15) and np.all(out["db_v"][:n_pix] == 0)
    assert np.allclose(out["nll"], -np.log(out["p"][np.arange(rows), out["y"]]), atol=1e-12)
    assert np.all(out["abs_dW"] >= np.abs(out["dW"]) - 1e-12)


def test_fp32_restatement_is_close_and_packed_layout():
    W, b_h, b_v = R.model(37, 10, 52)
    V, _ = R.labelled_batch(200, 37, 10)
    a, b = G.class_grad(W, b_h, b_v, V, 10), G.class_grad_fp32(W, b_h, b_v, V, 10)
    assert b["dW"].dtype == np.float32 and a["dW"].dtype == np.float64
    assert float(np.abs(b["g"] - a["g"]).max()) < 1e-5 and float(np.abs(b["p"] - a["p"]).max()) < 1e-4
    assert float((np.abs(b["dW"] - a["dW"]) / np.maximum(a["abs_dW"], 1.0)).max()) < 1e-5
    pk = G.packed(a)
    assert pk.shape == (47 * 52 + 52 + 47,) and np.array_equal(pk[:47 * 52].reshape(47, 52), a["dW"]) and np.array_equal(pk[-47:], a["db_v"])


def test_saturated_fixture_keeps_nll_finite_where_the_posterior_underflows():
    W, b_h, b_v = R.model(37, 10, 52, std=3.0)
    V, _ = R.labelled_batch(64, 37, 10)
    out = G.class_grad(W, b_h, b_v, V, 10)
    assert np.isfinite(out["nll"]).all() and out["nll"].max() > 40.0
    W, b_h, b_v = R.model(37, 10, 52, std=8.0)
    out = G.class_grad(W, b_h, b_v, V, 10)
    assert np.isfinite(out["nll"]).all() and out["nll"].max() > 104.0     # exp(-104) is zero in fp32: -log p_y would be infinite


def test_restatement_learns_the_prototypes():
    L = R.LEARN
    X, y = R.prototypes_data()
    W, b_h, b_v = R.learn_init()
    V = np.concatenate([X, R.one_hot(y, L["C"])], axis=1)
    ll0 = G.mean_log_posterior(W, b_h, b_v, V, L["C"])
    acc0 = float((R.predict(W, b_h, b_v, X, L["n_pix"]) == y).mean())
    W1, bh1, bv1, steps = G.disc_fit(W, b_h, b_v, V, L["C"], L["batch"], L["epochs"], L["lr"])
    ll = G.mean_log_posterior(W1, bh1, bv1, V, L["C"])
    acc = float((R.predict(W1, bh1, bv1, X, L["n_pix"]) == y).mean())
    print("mean log p(y | v) %.4f -> %.4f, accuracy %.4f -> %.4f" % (ll0, ll, acc0, acc))
    assert steps == L["epochs"] * 8
    assert ll >= -0.1 and acc >= 0.99


def test_hybrid_step_combines_the_two_gradients():
    W, b_h, b_v = R.model(37, 10, 52)
    V, _ = R.labelled_batch(64, 37, 10)
    dW, db_h, db_v, gen = G.hybrid_step(W, b_h, b_v, V, 10, 0.25, 42, 3)
    dsc = G.class_grad(W, b_h, b_v, V, 10)
    assert np.allclose(dW, dsc["dW"] + 0.25 * gen["dW"]) and np.allclose(db_v, dsc["db_v"] + 0.25 * gen["db_v"])
    assert np.allclose(db_h, dsc["db_h"] + 0.25 * gen["db_h"]) and np.abs(gen["dW"]).max() > 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kurbm.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define KURBM_ABI_VERSION 5" in text and lib.kurbm_abi_version() == 5
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [5, 14, 13, 14]
    # a null context is refused before anything else is looked at
    assert lib.kurbm_disc_workspace_bytes(None, 8, 8, 8, 3) == 0
    assert lib.kurbm_class_grad(None, None, 3, None, 8, 8, None, None, 8, None, None, None, 0, None) == -1
    assert lib.kurbm_disc_step(None, None, 3, None, 8, 8, None, 0.0, None, None, 0, None, None) == -1
    assert lib.kurbm_disc_epoch(None, None, 3, None, 8, 8, 4, None, 0.0, None, None, 0, None, None) == -1


# ---- host logic --------------------------------------------------------------------------------------------------------------
class FakeEngine:
    """What fit() of a non-generative objective asks of an engine; every call is recorded."""

    def __init__(self, n_vis, n_hid):
        self.n_vis, self.n_hid, self.device = n_vis, n_hid, torch.device("cpu")
        self.calls = []

    def v_pieces(self, v):
        return 1

    def check_status(self):
        pass

    def disc_step(self, v, rows, row_start, lr, n_labels, gen_weight=0.0, seed=0, step=0, k=1, chain=0, v_chain=None, row0=0,
                  momentum=None, want_nll=False, ws=None):
        self.calls.append(("step", rows, row_start, lr, n_labels, gen_weight, seed, step, k, v_chain is not None, momentum))
        return torch.full((1,), 0.5 + step) if want_nll else None

    def disc_epoch(self, v, n_rows, batch_size, lr, n_labels, gen_weight=0.0, seed=0, step0=0, k=1, v_chain=None, row_start=0,
                   momentum=None, want_nll=False, ws=None):
        self.calls.append(("epoch", n_rows, batch_size, lr, n_labels, gen_weight, seed, step0, k, v_chain is not None, momentum))
        return (n_rows + batch_size - 1) // batch_size

    def cd_epoch(self, *a, **kw):
        self.calls.append(("cd_epoch", kw.get("n_labels")))
        return 3

    def class_logits(self, v, n_labels, rows=None, row_start=0, want_prob=True, ws=None):
        lg = DeviceMatrix.zeros(v.rows, n_labels, self.device)
        lg.t[:, 1] = 1.0
        return lg, None


def fake_rbm(n_pix=6, C=3, n_hid=4, **kw):
    r = RBM(dict(HPS), n_hid, mode=MODE_VISIBLE_BERNOULLI, seed=11, n_labels=C, **kw)
    r._dev = FakeEngine(n_pix + C, n_hid)
    r.input_shape, r.output_shape, r.built = (None, n_pix + C), (None, n_hid), True
    return r


X10, Y10 = np.zeros((10, 6), np.float32), [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]


def test_objective_and_gen_weight_validation():
    with pytest.raises(ValueError, match="objective"):
        RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3, objective="supervised")
    for obj in ("discriminative", "hybrid"):
        with pytest.raises(ValueError, match="needs a label RBM"):
            RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, objective=obj)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gen_weight"):
            RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3, objective="hybrid", gen_weight=bad)
    # gen_weight is read by 'hybrid' only
    assert RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3, objective="discriminative", gen_weight=0.0).gen_weight == 0.0
    r = RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI, n_labels=3)
    assert r.objective == "generative" and r.gen_weight == 0.01
    assert RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI).objective == "generative"
    r = RBM(dict(HPS, objective="hybrid", gen_weight=0.05, n_labels=3), 4, mode=MODE_VISIBLE_BERNOULLI)       # hps keys work too
    assert r.objective == "hybrid" and r.gen_weight == 0.05


def test_epoch_path_step_path_and_the_update_counter(capsys):
    r = fake_rbm(objective="discriminative")
    r.fit(X10, verbose=0, y=Y10)
    # two epochs, each ONE epoch call on batches of 4 (4 + 4 + 2); the counter advances by one per batch
    assert r._dev.calls == [("epoch", 10, 4, 0.1, 3, 0.0, 11, 0, 1, False, None), ("epoch", 10, 4, 0.1, 3, 0.0, 11, 3, 1, False, None)]
    assert r._update_count == 6 and r._epochs_done == 2 and r.last_scores == []
    s = fake_rbm(objective="discriminative")
    s.fit(X10, verbose=1, y=Y10)
    assert [c[:4] for c in s._dev.calls] == [("step", 4, 0, 0.1), ("step", 4, 4, 0.1), ("step", 2, 8, 0.1)] * 2
    assert [c[7] for c in s._dev.calls] == [0, 1, 2, 3, 4, 5] and s._update_count == 6
    # one score per batch, the step's mean nll, in the reference's format
    assert s.last_scores == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5]
    out = capsys.readouterr().out
    assert "1/3, score: 0.500000" in out and "3/3, score: 5.500000" in out and out.count("score:") == 6


def test_hybrid_and_momentum_reach_the_engine():
    r = fake_rbm(objective="hybrid", gen_weight=0.02, cd_k=2, momentum=[0.5, 0.9], weight_decay=1e-3)
    r.fit(X10, verbose=0, y=Y10)
    assert r._dev.calls == [("epoch", 10, 4, 0.1, 3, 0.02, 11, 0, 2, False, (0.5, 1e-3)), ("epoch", 10, 4, 0.1, 3, 0.02, 11, 3, 2, False, (0.9, 1e-3))]
    # the default objective makes the calls of before
    g = fake_rbm()
    g.fit(X10, verbose=0, y=Y10)
    assert [c[0] for c in g._dev.calls] == ["cd_epoch", "cd_epoch"] and g._dev.calls[0][1] == 3


def test_refused_fits_reach_no_engine_call(monkeypatch):
    from keras_unsupervised_amd.ebm import dp
    r = fake_rbm(objective="discriminative")
    with pytest.raises(ValueError, match="labels must be integers"):
        r.fit(X10, verbose=0, y=[3] * 10)
    with pytest.raises(ValueError, match="one-hot"):
        r.fit(np.zeros((10, 9), np.float32), verbose=0)
    s = fake_rbm(objective="hybrid", update_mode="reference_sequential")
    with pytest.raises(ValueError, match="fused"):
        s.fit(X10, verbose=0, y=Y10)
    monkeypatch.setattr(dp, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="no data-parallel fit"):
        r.fit(X10, verbose=0, y=Y10)
    assert r._dev.calls == [] and s._dev.calls == [] and r._update_count == 0 and s._update_count == 0


def test_class_log_likelihood_on_the_double():
    r = fake_rbm(objective="discriminative")
    ll = r.class_log_likelihood(np.zeros((5, 6), np.float32), [1, 1, 0, 2, 1])
    lse = np.log(np.exp(1.0) + 2.0)
    assert abs(ll - ((3 * 1.0 + 2 * 0.0) / 5 - lse)) < 1e-12
    with pytest.raises(ValueError, match="labels"):
        r.class_log_likelihood(np.zeros((5, 6), np.float32), [1, 1, 0, 3, 1])
    with pytest.raises(ValueError, match="label RBM"):
        plain = fake_rbm()
        plain.n_labels = 0
        plain.class_log_likelihood(np.zeros((5, 6), np.float32), [0] * 5)


def test_config_and_checkpoint_keys(tmp_path):
    from keras_unsupervised_amd.ebm import checkpoint
    r = RBM(HPS, 7, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=3, n_labels=10, objective="hybrid", gen_weight=0.05)
    cfg = r.get_config()
    assert cfg["objective"] == "hybrid" and cfg["gen_weight"] == 0.05
    r2 = RBM(**cfg)
    assert r2.objective == "hybrid" and r2.gen_weight == 0.05 and r2.get_config() == cfg
    assert RBM(HPS, 7, mode=MODE_VISIBLE_BERNOULLI).get_config()["objective"] == "generative"
    # the checkpoint's JSON carries both keys (the writer needs only get_weights / get_config of a built object)
    f = fake_rbm(objective="hybrid", gen_weight=0.05)
    f.get_weights = lambda: (np.zeros((9, 4), np.float32), np.zeros(4, np.float32), np.zeros(9, np.float32))
    jpath, _ = checkpoint.save_rbm(f, str(tmp_path / "ck"))
    meta = json.load(open(jpath))
    assert meta["config"]["objective"] == "hybrid" and meta["config"]["gen_weight"] == 0.05
    # ... and a checkpoint written before them builds a generative RBM
    old = {k: v for k, v in meta["config"].items() if k not in ("objective", "gen_weight")}
    assert RBM(**old).objective == "generative"
