"""CPU tier of DBN fine-tuning: the yardstick of tests/test_gpu_backprop.py -- the float64 restatement of tests/backprop_ref.py must
agree with central differences of sum log p(y | v) and with torch.autograd in float64 for every parameter block, must learn the
prototype classes and move the lower layers -- the C ABI's new symbols, the margin of the GPU tier's relu fixtures, and the host
logic of DBN.fine_tune on engine doubles: the call order per batch, the remainder batch, the defaults from hps, the momentum
schedule, the update counters.  A call the host refuses reaches no engine call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # backprop_ref.py and its neighbours live beside this file
import backprop_ref as B
import labels_ref as R
from keras_unsupervised_amd import _lib
from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, RBM
from keras_unsupervised_amd.ebm.engine import DeviceMatrix

NEW_SYMBOLS = ("kurbm_backprop_workspace_bytes", "kurbm_backprop_delta", "kurbm_backprop_layer", "kurbm_disc_backprop")
# the 7 -> 6 -> 5 stack under a 5 + 3 -> 4 top; per bottom activation the seed for which no relu pre-activation is within 1e-3 of zero
SIZES, TOP_HID, C, ROWS = (7, 6, 5), 4, 3, 9
GRAD_SEEDS = {B.ACT_SIGMOID: 1, B.ACT_RELU: 0}


def _grad_problem(act):
    lower, top = B.stack(SIZES, TOP_HID, C, (act, act), seed=GRAD_SEEDS[act])
    V, y = B.batch(ROWS, SIZES[0], C, seed=GRAD_SEEDS[act], binary=act != B.ACT_RELU)
    lower = [(W.astype(np.float64), b.astype(np.float64), a) for W, b, a in lower]
    top = tuple(x.astype(np.float64) for x in top)
    return lower, top, V.astype(np.float64), y


def _blocks(lower, top, s):
    """(name, parameter array, its gradient) for every parameter block of the stack."""
    out = []
    for l, ((W, b, _), sl) in enumerate(zip(lower, s["layers"])):
        out += [("W%d" % (l + 1), W, sl["dW"]), ("b_h%d" % (l + 1), b, sl["db_h"])]
    return out + [("W_top", top[0], s["top"]["dW"]), ("b_h_top", top[1], s["top"]["db_h"]), ("b_v_top", top[2], s["top"]["db_v"])]


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
def test_gradient_equals_central_differences(act):
    lower, top, V, y = _grad_problem(act)
    if act == B.ACT_RELU:
        assert B.min_abs_pre(lower, V) > B.RELU_MARGIN, "fixture: a relu pre-activation sits at the kink (pick another seed)"
    s = B.grad(lower, top, C, V, y)
    eps, worst = 1e-5, 0.0
    for name, x, g in _blocks(lower, top, s):        # (x is the array inside lower / top: perturbed in place, restored)
        for idx in np.ndindex(x.shape):
            keep = x[idx]
            x[idx] = keep + eps
            up = B.total_log_posterior(lower, top, C, V, y)
            x[idx] = keep - eps
            num = (up - B.total_log_posterior(lower, top, C, V, y)) / (2 * eps)
            x[idx] = keep
            dev = abs(num - g[idx]) / max(1.0, abs(g[idx]))
            worst = max(worst, dev)
            assert dev <= 1e-6, (name, idx, num, g[idx])        # (the bar of tests/test_classgrad_host.py)
    print("worst deviation from central differences %.3g" % worst)
    # the pieces are consistent with one another
    for sl in s["layers"]:
        assert np.all(sl["db_v"] == 0) and np.all(sl["abs_dW"] >= np.abs(sl["dW"]) - 1e-12)
    assert "e_in" not in s["layers"][0] and s["layers"][1]["e_in"].shape == (ROWS, SIZES[1])


def _torch_grads(lower, top, V, y):
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    prm = [(t64(W), t64(b), act) for W, b, act in lower]
    W, b_h, b_v = [t64(a) for a in top]
    x = torch.tensor(V)
    for Wl, bl, act in prm:
        pre = x @ Wl + bl
        x = torch.sigmoid(pre) if act == B.ACT_SIGMOID else torch.relu(pre)
    n_pix = W.shape[0] - C
    o = (x @ W[:n_pix] + b_h)[:, None, :] + W[n_pix:][None, :, :]
    logits = torch.nn.functional.softplus(o).sum(dim=2) + b_v[n_pix:]
    loss = torch.log_softmax(logits, dim=1)[torch.arange(V.shape[0]), torch.tensor(y)].sum()
    loss.backward()
    out = []
    for Wl, bl, _ in prm:
        out += [Wl.grad.numpy(), bl.grad.numpy()]
    return out + [W.grad.numpy(), b_h.grad.numpy(), b_v.grad.numpy()], float(loss.detach())


@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
def test_gradient_equals_torch_autograd_in_float64(act):
    lower, top, V, y = _grad_problem(act)
    if act == B.ACT_RELU:
        assert B.min_abs_pre(lower, V) > B.RELU_MARGIN
    s = B.grad(lower, top, C, V, y)
    want, loss = _torch_grads(lower, top, V, y)
    assert abs(loss - B.total_log_posterior(lower, top, C, V, y)) <= 1e-12 * max(1.0, abs(loss))
    worst = 0.0
    for (name, _, g), w in zip(_blocks(lower, top, s), want):
        # two float64 evaluations of sums of at most rows x C x n_hid terms of order one: 1e-12 is a thousand roundings
        dev = float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max())
        worst = max(worst, dev)
        assert dev <= 1e-12, (name, dev)
    print("worst deviation from torch.autograd %.3g" % worst)


def test_fp32_restatement_is_close():
    lower, top = B.stack((70, 36, 20), 24, 5, (B.ACT_SIGMOID, B.ACT_RELU), seed=3)
    V, y = B.batch(64, 70, 5, seed=3)
    a, b = B.grad(lower, top, 5, V, y), B.grad(lower, top, 5, V, y, dt=np.float32)
    for sa, sb in zip(a["layers"], b["layers"]):
        assert sb["dW"].dtype == np.float32 and sa["dW"].dtype == np.float64
        assert float((np.abs(sb["dW"] - sa["dW"]) / np.maximum(sa["abs_dW"], 1.0)).max()) < 1e-4
        assert float(np.abs(sb["delta"] - sa["delta"]).max()) < 1e-4
    # a layer given its planes restates the stack's own layer
    xs, e = a["xs"], a["top"]["e_in"]
    one = B.layer_backward(lower[1][0], lower[1][2], xs[1], xs[2], e)
    assert np.array_equal(one["dW"], a["layers"][1]["dW"]) and np.array_equal(one["e_in"], a["layers"][1]["e_in"])
    assert np.array_equal(B.site(e, xs[2], B.ACT_LINEAR), e)


def test_restatement_learns_the_prototypes_and_moves_the_lower_layers():
    X, y = R.prototypes_data()
    lower, top = B.stack((32, 24, 16), 16, 4, (B.ACT_SIGMOID, B.ACT_SIGMOID), seed=2)        # fixed weights, N(0, 0.3)
    ll0, acc0 = B.mean_log_posterior(lower, top, 4, X, y), float((B.predict(lower, top, 4, X) == y).mean())
    lower1, top1, steps, _ = B.fine_tune(lower, top, 4, X, y, 64, 10, 0.01)
    ll, acc = B.mean_log_posterior(lower1, top1, 4, X, y), float((B.predict(lower1, top1, 4, X) == y).mean())
    print("mean log p(y | v) %.4f -> %.4f, accuracy %.4f -> %.4f" % (ll0, ll, acc0, acc))
    assert steps == 10 * 8
    assert ll > ll0 and acc >= acc0
    for (W0, b0, _), (W1, b1, _) in zip(lower, lower1):
        assert np.abs(W1 - W0).max() > 1e-3 and np.abs(b1 - b0).max() > 1e-4
    # momentum and weight decay take the other branch of the loop and learn too
    lower2, top2, _, _ = B.fine_tune(lower, top, 4, X, y, 64, 5, 0.002, momentum=[0.5, 0.9], weight_decay=1e-3)
    assert B.mean_log_posterior(lower2, top2, 4, X, y) > ll0


@pytest.mark.parametrize("momentum,decay", [(0.0, 0.0), (B.TRAJ["momentum"], B.TRAJ["weight_decay"])], ids=["plain", "momentum"])
def test_relu_fixtures_of_the_gpu_trajectory_keep_their_margin(momentum, decay):
    T = B.TRAJ
    lower, top, V, y = B.traj_problem(B.ACT_RELU)
    _, _, steps, margin = B.fine_tune(lower, top, T["C"], V, y, T["batch"], T["epochs"], T["lr"], momentum=momentum, weight_decay=decay)
    print("smallest |pre-activation| on the trajectory %.3g" % margin)
    assert steps == T["epochs"] * 4 and margin > B.RELU_MARGIN


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_refuse_a_null_context():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kurbm.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define KURBM_ABI_VERSION 5" in text and lib.kurbm_abi_version() == 5
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [4, 14, 16, 13]
    assert lib.kurbm_backprop_workspace_bytes(None, 8, 8, 8) == 0
    assert lib.kurbm_backprop_delta(None, None, 8, None, 8, 8, 8, 0, None, 8, None, None, 0, None) == -1
    assert lib.kurbm_backprop_layer(None, None, 0, None, 8, None, 8, None, 8, 8, None, None, 8, None, 0, None) == -1
    assert lib.kurbm_disc_backprop(None, None, 3, None, 8, 8, None, None, 8, None, None, 0, None) == -1


# ---- host logic --------------------------------------------------------------------------------------------------------------
class FakeEngine:
    """What DBN.fine_tune asks of a layer's engine; every call of every layer is recorded in ONE shared log."""

    def __init__(self, name, n_vis, n_hid, log):
        self.name, self.n_vis, self.n_hid, self.device, self.calls = name, n_vis, n_hid, torch.device("cpu"), log
        self.delta = "delta-" + name

    def check_status(self):
        self.calls.append((self.name, "status"))

    def probs_into(self, x, rows, row_start, act, out, out_row=0):
        self.calls.append((self.name, "forward", rows, row_start, act, x.cols, out.cols))
        return out

    def disc_backprop(self, v, n_labels, rows=None, row_start=0, e_in=None, want_nll=False, ws=None):
        self.calls.append((self.name, "disc_backprop", rows, row_start, n_labels, None if e_in is None else e_in.cols,
                           v.t[:rows, self.n_vis - n_labels:self.n_vis].argmax(dim=1).tolist() if row_start == 0 else None))
        self.steps = getattr(self, "steps", 0) + 1
        return self.delta, (torch.full((1,), 0.25 * self.steps) if want_nll else None)

    def backprop_layer(self, act, x_in, x_out, e, rows=None, row_start=0, e_in=None, ws=None):
        self.calls.append((self.name, "backprop_layer", rows, row_start, act, x_in.cols, x_out.cols, e.cols, None if e_in is None else e_in.cols))
        return self.delta

    def apply_delta(self, lr, which=7, delta=None, compute=None, momentum=None):
        self.calls.append((self.name, "apply", lr, which, delta, momentum))


def fake_dbn(sizes=(6, 5, 4), top_hid=3, n_labels=3, modes=(MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN), hps=None):
    log, dbn = [], DBN()
    hps = hps or {"batch_size": 4, "epochs": 2, "lr": 0.1}
    for i, (a, b, mode) in enumerate(zip(sizes[:-1], sizes[1:], modes)):
        r = RBM({"batch_size": 99, "epochs": 99, "lr": 9.0}, b, name="l%d" % (i + 1), mode=mode, seed=1)
        r._dev, r.input_shape, r.output_shape, r.built = FakeEngine(r.name, a, b, log), (None, a), (None, b), True
        dbn.add_stack(r)
    t = RBM(dict(hps), top_hid, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=1, n_labels=n_labels)
    nv = sizes[-1] + n_labels
    t._dev, t.input_shape, t.output_shape, t.built = FakeEngine("top", nv, top_hid, log), (None, nv), (None, top_hid), True
    dbn.add_stack(t)
    return dbn, log


X10, Y10 = np.zeros((10, 6), np.float32), [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]


def _batch_calls(rows, lo, lr, mom, labels):
    """The calls of one batch on the 6 -> 5 -> 4 stack (sigmoid, relu) under the 4 + 3 -> 3 top, in order."""
    return [("l1", "forward", rows, lo, B.ACT_SIGMOID, 6, 5), ("l2", "forward", rows, 0, B.ACT_RELU, 5, 7),
            ("top", "disc_backprop", rows, 0, 3, 4, labels),
            ("l2", "backprop_layer", rows, 0, B.ACT_RELU, 5, 7, 4, 5), ("l1", "backprop_layer", rows, lo, B.ACT_SIGMOID, 6, 5, 5, None),
            ("l1", "apply", lr, 3, "delta-l1", mom), ("l2", "apply", lr, 3, "delta-l2", mom), ("top", "apply", lr, 7, "delta-top", mom)]


def test_call_order_remainder_batch_defaults_and_counters(capsys):
    dbn, log = fake_dbn()
    assert dbn.fine_tune(X10, Y10, verbose=0) is None
    # epochs, lr and batch_size from the TOP layer's hps: two epochs of 4 + 4 + 2 rows, the remainder last; one status read at the end
    want = []
    for _ in range(2):
        for lo, rows in ((0, 4), (4, 4), (8, 2)):
            want += _batch_calls(rows, lo, 0.1, None, Y10[lo:lo + rows])
    assert [c for c in log if c[1] != "apply"] == [c for c in want if c[1] != "apply"] + [("top", "status")]
    assert [c[:5] for c in log if c[1] == "apply"] == [c[:5] for c in want if c[1] == "apply"]
    assert all(c[5] is None for c in log if c[1] == "apply")          # no momentum keyword's value without either term
    assert [layer._update_count for layer in dbn._layers()] == [6, 6, 6]
    assert capsys.readouterr().out == "" and dbn.last_scores == []
    # explicit arguments override the hps; verbose = 1 prints each batch's mean nll in fit()'s format
    dbn2, log2 = fake_dbn()
    dbn2.fine_tune(X10, Y10, epochs=1, lr=0.5, batch_size=5, verbose=1)
    assert [c[2:4] for c in log2 if c[1] == "forward" and c[0] == "l1"] == [(5, 0), (5, 5)]
    assert all(c[2] == 0.5 for c in log2 if c[1] == "apply") and [layer._update_count for layer in dbn2._layers()] == [2, 2, 2]
    out = capsys.readouterr().out
    assert dbn2.last_scores == [0.25, 0.5] and "1/2, score: 0.250000" in out and "2/2, score: 0.500000" in out


def test_momentum_schedule_by_epoch_and_weight_decay():
    dbn, log = fake_dbn()
    dbn.fine_tune(X10, Y10, epochs=3, momentum=[0.5, 0.9], weight_decay=1e-3, verbose=0)
    moms = [c[5] for c in log if c[1] == "apply"]
    assert moms == [(0.5, 1e-3)] * 9 + [(0.9, 1e-3)] * 18            # three applies per batch, three batches per epoch
    dbn, log = fake_dbn()
    dbn.fine_tune(X10, Y10, epochs=1, momentum=0.0, weight_decay=2e-3, verbose=0)
    assert all(c[5] == (0.0, 2e-3) for c in log if c[1] == "apply")
    for bad in (dict(momentum=1.0), dict(momentum=[]), dict(momentum=[0.5, -0.1]), dict(weight_decay=-1.0)):
        dbn, log = fake_dbn()
        with pytest.raises(ValueError, match="momentum|weight_decay"):
            dbn.fine_tune(X10, Y10, verbose=0, **bad)
        assert log == []


def test_one_layer_dbn_steps_on_the_joined_matrix():
    log, dbn = [], DBN()
    t = RBM({"batch_size": 4, "epochs": 1, "lr": 0.1}, 3, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=1, n_labels=3)
    t._dev, t.input_shape, t.output_shape, t.built = FakeEngine("top", 9, 3, log), (None, 9), (None, 3), True
    dbn.add_stack(t)
    dbn.fine_tune(X10, Y10, verbose=0)
    assert [c[:5] for c in log if c[1] == "disc_backprop"] == [("top", "disc_backprop", 4, 0, 3), ("top", "disc_backprop", 4, 4, 3),
                                                               ("top", "disc_backprop", 2, 8, 3)]
    assert all(c[5] is None for c in log if c[1] == "disc_backprop") and [c[1] for c in log].count("apply") == 3
    assert t._update_count == 3


def test_refusals_reach_no_engine_call(monkeypatch):
    from keras_unsupervised_amd.ebm import dp
    plain, log0 = DBN(), []
    r = RBM({"batch_size": 4, "epochs": 1, "lr": 0.1}, 5, name="l1", mode=MODE_VISIBLE_BERNOULLI)
    r._dev, r.input_shape, r.output_shape, r.built = FakeEngine("l1", 6, 5, log0), (None, 6), (None, 5), True
    plain.add_stack(r)
    with pytest.raises(ValueError, match="label RBM"):
        plain.fine_tune(X10, Y10, verbose=0)
    with pytest.raises(ValueError, match="label RBM"):
        plain.class_log_likelihood(X10, Y10)
    with pytest.raises(ValueError, match="Any rbm layer"):
        DBN().fine_tune(X10, Y10)
    dbn, log = fake_dbn()
    dbn._layers()[1].built = False
    with pytest.raises(ValueError, match="built"):
        dbn.fine_tune(X10, Y10, verbose=0)
    dbn, log = fake_dbn()
    with pytest.raises(ValueError, match="labels must be integers"):
        dbn.fine_tune(X10, [3] * 10, verbose=0)
    with pytest.raises(ValueError, match="labels must be integers"):
        dbn.fine_tune(X10, np.linspace(0, 1, 10), verbose=0)
    with pytest.raises(ValueError, match="9 labels for 10 rows"):
        dbn.fine_tune(X10, Y10[:9], verbose=0)
    with pytest.raises(ValueError, match="columns"):
        dbn.fine_tune(np.zeros((10, 7), np.float32), Y10, verbose=0)
    monkeypatch.setattr(dp, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="data-parallel"):
        dbn.fine_tune(X10, Y10, verbose=0)
    assert log == [] and log0 == [] and all(layer._update_count == 0 for layer in dbn._layers())


def test_class_log_likelihood_goes_through_the_lower_layers():
    dbn, _ = fake_dbn()
    seen = []
    for layer in dbn._layers()[:-1]:
        layer.hidden_probs = (lambda name, n_out: lambda v: (seen.append((name, v.cols)), DeviceMatrix.zeros(v.rows, n_out, torch.device("cpu")))[1])(
            layer.name, layer._dev.n_hid)
    dbn._layers()[-1].class_log_likelihood = lambda v, y: (seen.append(("top", v.cols, list(y))), -0.5)[1]
    assert dbn.class_log_likelihood(X10, Y10) == -0.5
    assert seen == [("l1", 6), ("l2", 5), ("top", 4, Y10)]
