"""CPU tier: the yardstick of tests/test_gpu_gibbs.py -- the float64 restatement of tests/gibbs_ref.py must itself sample the
enumerated p(v) of a small RBM, free and clamped, and its flagged-chain counts are what the GPU tier's cap rests on -- and the
host logic of RBM.gibbs / RBM.sample / DBN.sample on an engine double: refusals, the chain0 bookkeeping, the (kept, chain)
order, the call order of a DBN dream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # gibbs_ref.py lives beside this file
import gibbs_ref as R
from keras_unsupervised_amd import _lib
from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, RBM
from keras_unsupervised_amd.ebm import engine as E
from keras_unsupervised_amd.ebm.engine import DeviceMatrix

HPS = {"batch_size": 4, "epochs": 1, "lr": 0.1}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def test_enumeration_is_a_distribution():
    W, b_h, b_v = R.dist_params()
    p = R.exact_pv(W, b_h, b_v)
    assert p.shape == (64,) and abs(p.sum() - 1.0) <= 1e-12 and p.min() > 0
    # against the joint, written out: p(v) = sum_h exp(v.W.h + b_v.v + b_h.h) / Z
    Sv, Sh = R.state_matrix(6), R.state_matrix(5)
    e = (Sv @ W.astype(np.float64)) @ Sh.T + (Sv @ b_v.astype(np.float64))[:, None] + (Sh @ b_h.astype(np.float64))[None, :]
    joint = np.exp(e).sum(axis=1)
    assert np.max(np.abs(p - joint / joint.sum())) <= 1e-12
    pc = R.exact_pv(W, b_h, b_v, R.DIST_CLAMP, R.DIST_VALUES)
    ok = (Sv[:, 0] == 1.0) & (Sv[:, 3] == 0.0)
    assert abs(pc.sum() - 1.0) <= 1e-12 and np.all(pc[~ok] == 0.0) and np.max(np.abs(pc[ok] - p[ok] / p[ok].sum())) <= 1e-12
    assert np.array_equal(R.state_index(Sv), np.arange(64))


@pytest.mark.parametrize("clamped", [False, True])
def test_restatement_samples_the_model(clamped):
    """6 x 5, 8192 chains, 200 sweeps: every one of the 64 visible states inside 4 sigma + 1 / N of its enumerated probability
    (of the conditional, with visibles {0, 3} clamped)."""
    W, b_h, b_v = R.dist_params()
    p = R.exact_pv(W, b_h, b_v, *((R.DIST_CLAMP, R.DIST_VALUES) if clamped else ()))
    v = R.dist_run(clamped)
    assert v.shape == (R.DIST_CHAINS, 6) and set(np.unique(v)) <= {0.0, 1.0}
    if clamped:
        assert np.all(v[:, 0] == 1.0) and np.all(v[:, 3] == 0.0)
    bad, f = R.band_violations(v, p, 4.0)
    assert bad.size == 0, "states %s: f = %s, p = %s" % (bad, f[bad], p[bad])


@pytest.mark.parametrize("seed", [7, 8])
def test_restatement_flags_few_chains(seed):
    """tests/test_gpu_gibbs.py lets at most 10 % of the 200 chains of its runs be flagged (expected: about 2 % = 8 sweeps x 106
    draws x 2e-5); the restatement's own runs must stay below that cap."""
    for kw in ({}, {"burn_in": 2, "thin": 3, "n_keep": 3}, {"clamped": True}):
        v, p, flagged = R.free_run(seed, **kw)
        print("seed %d %s: %d of %d chains flagged" % (seed, kw, int(flagged.sum()), flagged.size))
        assert flagged.sum() <= 0.10 * flagged.size
        assert set(np.unique(v)) <= {0.0, 1.0} and p.min() >= 0.0 and p.max() <= 1.0
    _, _, flagged = R.gauss_run(seed)
    assert flagged.sum() <= 0.10 * flagged.size


def test_restatement_keeps_the_right_sweeps():
    """Kept sample j is v_{burn_in + j thin}: the kept planes of (2, 3, 3) are sweeps 2, 5, 8 of the plain eight-sweep run, and
    clamped columns hold v_init in samples and probabilities."""
    W, b_h, b_v = R.free_params(7)
    v0 = R.free_init(7)[:16]
    kept, _, _ = R.run(W, b_h, b_v, v0, 0, 7, burn_in=2, thin=3, n_keep=3)
    for j, T in enumerate((2, 5, 8)):
        assert np.array_equal(kept[j], R.run(W, b_h, b_v, v0, 0, 7, burn_in=T)[0][0])
    vc, pc, _ = R.run(W, b_h, b_v, v0, 0, 7, burn_in=2, thin=3, n_keep=3, clamp=R.CLAMP_COLS)
    for j in range(3):
        assert np.array_equal(vc[j][:, R.CLAMP_COLS], v0[:, R.CLAMP_COLS]) and np.array_equal(pc[j][:, R.CLAMP_COLS], v0[:, R.CLAMP_COLS])
    assert not np.array_equal(vc[2], kept[2])
    # chain indices, not positions, name the draws: rows 4 .. 7 of a run from chain0 = 0 are a run from chain0 = 4
    a = R.run(W, b_h, b_v, v0[:8], 0, 7, burn_in=3)[0][0]
    b = R.run(W, b_h, b_v, v0[4:8], 4, 7, burn_in=3)[0][0]
    assert np.array_equal(a[4:], b)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kurbm.h")).read()
    lib = _lib.load()
    for name in ("kurbm_gibbs_workspace_bytes", "kurbm_gibbs_run"):
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define KURBM_STREAM_GIBBS_H 0x210u" in text and "#define KURBM_STREAM_GIBBS_V 0x211u" in text
    assert (E.STREAM_GIBBS_H, E.STREAM_GIBBS_V) == (R.STREAM_GIBBS_H, R.STREAM_GIBBS_V) == (0x210, 0x211)
    assert len(_lib.SIGNATURES["kurbm_gibbs_run"][1]) == 22 and lib.kurbm_abi_version() == 5
    # a null context is refused by the size query, and by the run before it looks at anything else
    assert lib.kurbm_gibbs_workspace_bytes(None, 8, 8, 8, 1, 0) == 0
    assert lib.kurbm_gibbs_run(None, None, None, 0, None, 1, 8, 8, 0, 0, 0, 1, 1, 1, None, None, None, 8, 0, None, 0, None) == -1


def test_clamp_mask():
    assert E.clamp_mask([0, 3], 5).tolist() == [1, 0, 0, 1, 0]
    assert E.clamp_mask(np.array([True, False, True]), 3).tolist() == [1, 0, 1]
    assert E.clamp_mask([], 4).tolist() == [0, 0, 0, 0]
    for bad in ([5], [-1], np.array([True, False]), [0.5]):
        with pytest.raises(ValueError):
            E.clamp_mask(bad, 5)


# ---- host logic on an engine double ---------------------------------------------------------------------------------------
class FakeEngine:
    """What RBM.gibbs / sample / hidden_probs ask of a DeviceRBM, on the CPU: gibbs_run records its arguments and returns
    n_keep * rows rows whose column 0 is the row's index in (kept, chain) order and column 1 the chain's index."""

    def __init__(self, n_vis, n_hid, log=None, name=""):
        self.n_vis, self.n_hid, self.device = n_vis, n_hid, torch.device("cpu")
        self.b_v = torch.zeros(n_vis)
        self.calls, self.log, self.name = [], log if log is not None else [], name

    def philox_uniform(self, rows, cols, seed, stream_id, step, row0=0):
        self.calls.append(("philox", rows, cols, seed, stream_id, step, row0))
        m = DeviceMatrix.zeros(rows, cols, self.device)
        m.view().fill_(0.25)
        return m

    def gibbs_run(self, v, burn_in=1, thin=1, n_keep=1, chain0=0, seed=0, mode=0, clamp=None, want_prob=False, ws=None):
        self.calls.append(("gibbs", v.rows, burn_in, thin, n_keep, chain0, seed, mode, clamp, want_prob))
        self.log.append((self.name, "gibbs"))
        self.last_init = v.view().clone()
        out = DeviceMatrix.zeros(n_keep * v.rows, self.n_vis, self.device)
        out.t[:, 0] = torch.arange(n_keep * v.rows, dtype=torch.float32)
        out.t[:, 1] = torch.arange(n_keep * v.rows, dtype=torch.float32) % v.rows
        prob = None
        if want_prob:
            prob = DeviceMatrix.zeros(n_keep * v.rows, self.n_vis, self.device)
            prob.t[:, 0] = 0.5
        return out, prob

    def half_step(self, direction, x, rows, row_start, act, noise, seed, stream_id, step, row0=0, want_sample=True,
                  want_prob=False, want_u=False):
        self.calls.append(("half", direction, rows, act, noise, step, want_sample, want_prob))
        self.log.append((self.name, direction, noise))
        m = DeviceMatrix.zeros(rows, self.n_hid if direction == "vh" else self.n_vis, self.device)
        return {"sample": m if want_sample else None, "prob": m if want_prob else None, "u": None}


def fake_rbm(n_vis=6, n_hid=4, mode=MODE_VISIBLE_BERNOULLI, seed=11, log=None, name=""):
    r = RBM(HPS, n_hid, mode=mode, seed=seed, name=name)
    r._dev = FakeEngine(n_vis, n_hid, log, name)
    r.input_shape, r.output_shape, r.built = (None, n_vis), (None, n_hid), True
    return r


def test_unbuilt_and_bad_arguments_are_refused():
    r = RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI)
    v = np.zeros((3, 6), np.float32)
    for call in (lambda: r.gibbs(v), lambda: r.sample(4), lambda: r.visible_probs(np.zeros((3, 4), np.float32))):
        with pytest.raises(ValueError, match="needs a built RBM"):
            call()
    r = fake_rbm()
    for call, what in ((lambda: r.gibbs(v, n_steps=0), "n_steps"), (lambda: r.gibbs(np.zeros((3, 5), np.float32)), "columns"),
                       (lambda: r.gibbs(np.zeros((0, 6), np.float32)), "empty"), (lambda: r.sample(0), "positive"),
                       (lambda: r.sample(4, n_chains=0), "positive"), (lambda: r.sample(4, burn_in=0), "burn_in"),
                       (lambda: r.sample(4, thin=0), "thin"), (lambda: r.sample(4, clamp=[0]), "clamp needs init"),
                       (lambda: r.sample(4, init=np.zeros((3, 6), np.float32)), "init has shape"),
                       (lambda: r.sample(4, init=np.zeros((4, 5), np.float32)), "init has shape")):
        with pytest.raises(ValueError, match=what):
            call()
    assert r._dev.calls == [] and r._chains_used == 0 and r._update_count == 0 and r._call_count == 0


def test_chain_bookkeeping():
    r = fake_rbm()
    r.gibbs(np.zeros((5, 6), np.float32), n_steps=3)
    r.gibbs(np.zeros((4, 6), np.float32), seed=99, clamp=[1, 2], return_prob=True)
    r.sample(3, burn_in=7, thin=2)
    r.sample(2, burn_in=1)
    g = [c for c in r._dev.calls if c[0] == "gibbs"]
    #        rows, burn_in, thin, n_keep, chain0, seed, mode, clamp, want_prob
    assert g[0][1:] == (5, 3, 1, 1, 0, 11, MODE_VISIBLE_BERNOULLI, None, False)
    assert g[1][1:8] == (4, 1, 1, 1, 8, 99, MODE_VISIBLE_BERNOULLI) and g[1][8] == [1, 2] and g[1][9] is True
    assert g[2][1:] == (3, 7, 2, 1, 12, 11, MODE_VISIBLE_BERNOULLI, None, False)
    assert g[3][5] == 16 and r._chains_used == 20
    # the start of sample(): uniforms of the visible site at step 0 for exactly these chains; [0.25 < sigmoid(0)] = 1
    p = [c for c in r._dev.calls if c[0] == "philox"]
    assert p[0] == ("philox", 3, 6, 11, E.STREAM_GIBBS_V, 0, 12) and p[1][-1] == 16
    assert bool((r._dev.last_init == 1.0).all())
    assert r._update_count == 0 and r._call_count == 0 and r.last_ais is None
    gauss = fake_rbm(mode=MODE_VISIBLE_GAUSSIAN)
    gauss._dev.b_v = torch.arange(6, dtype=torch.float32)
    gauss.sample(2, burn_in=1)
    assert [c[0] for c in gauss._dev.calls] == ["gibbs"]
    assert torch.equal(gauss._dev.last_init, torch.arange(6, dtype=torch.float32).expand(2, 6))


def test_kept_chain_order_and_return_kinds():
    r = fake_rbm()
    out = r.sample(7, n_chains=3, burn_in=5, thin=2)
    assert r._dev.calls[-1][1:6] == (3, 5, 2, 3, 0)                 # three chains, ceil(7 / 3) = 3 kept states each
    assert isinstance(out, np.ndarray) and out.shape == (7, 6)
    assert out[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6] and out[:, 1].tolist() == [0, 1, 2, 0, 1, 2, 0]
    v, p = r.sample(4, n_chains=4, burn_in=1, init=torch.zeros(4, 6), return_prob=True)
    assert isinstance(v, torch.Tensor) and isinstance(p, torch.Tensor) and v.shape == p.shape == (4, 6) and float(p[0, 0]) == 0.5
    m = r.gibbs(DeviceMatrix.zeros(5, 6, torch.device("cpu")))
    assert isinstance(m, DeviceMatrix) and m.rows == 5
    assert not isinstance(r.gibbs(np.zeros((2, 6), np.float32)), list)


def test_probs_take_no_counter():
    r = fake_rbm()
    h = r.hidden_probs(np.zeros((3, 6), np.float32))
    v = r.visible_probs(np.zeros((3, 4), np.float32))
    assert h.shape == (3, 4) and v.shape == (3, 6) and r._call_count == 0
    assert r._dev.calls == [("half", "vh", 3, _lib.ACT_SIGMOID, _lib.NOISE_NONE, 0, False, True),
                            ("half", "hv", 3, _lib.ACT_SIGMOID, _lib.NOISE_NONE, 0, False, True)]
    g = fake_rbm(mode=MODE_VISIBLE_GAUSSIAN)
    g.hidden_probs(np.zeros((3, 6), np.float32)), g.visible_probs(np.zeros((3, 4), np.float32))
    assert [c[3] for c in g._dev.calls] == [_lib.ACT_RELU, _lib.ACT_LINEAR]


def test_dbn_sample_call_order():
    log = []
    dbn = DBN()
    dbn.add_stack(fake_rbm(8, 6, log=log, name="l0"))
    dbn.add_stack(fake_rbm(6, 5, log=log, name="l1"))
    dbn.add_stack(fake_rbm(5, 3, log=log, name="top"))
    out = dbn.sample(4, burn_in=9, thin=2)
    assert isinstance(out, np.ndarray) and out.shape == (4, 8)
    # the run in the top RBM, then down: inv_transform of l1, then of l0 -- the order of DBN.inv_transform
    assert log == [("top", "gibbs"), ("l1", "hv", _lib.NOISE_BERNOULLI), ("l0", "hv", _lib.NOISE_BERNOULLI)]
    assert dbn._layers()[2]._dev.calls[-1][1:5] == (4, 9, 2, 1)
    del log[:]
    out = dbn.sample(5, burn_in=1, n_chains=2, init=torch.zeros(2, 8), return_prob=True)
    assert isinstance(out, torch.Tensor) and out.shape == (5, 8)
    assert log == [("l0", "vh", _lib.NOISE_BERNOULLI), ("l1", "vh", _lib.NOISE_BERNOULLI), ("top", "gibbs"),
                   ("l1", "hv", _lib.NOISE_BERNOULLI), ("l0", "hv", _lib.NOISE_NONE)]
    assert dbn._layers()[2]._dev.calls[-1][1:5] == (2, 1, 100, 3)
    del log[:]
    dbn.transform_probs(np.zeros((3, 8), np.float32))
    assert log == [("l0", "vh", _lib.NOISE_NONE), ("l1", "vh", _lib.NOISE_NONE), ("top", "vh", _lib.NOISE_NONE)]
    unbuilt = DBN()
    unbuilt.add_stack(RBM(HPS, 4, mode=MODE_VISIBLE_BERNOULLI))
    with pytest.raises(ValueError, match="built"):
        unbuilt.sample(2)
