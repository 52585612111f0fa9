"""GPU tier of the softmax label units (include/kurbm.h: kurbm_label_sample, kurbm_cd_step_labels, kurbm_cd_epoch_labels,
kurbm_class_logits; csrc/kurbm_labels.hip) against the float64 restatement of tests/labels_ref.py, whose own standing and whose
fixtures' margins the CPU tier (tests/test_labels_host.py) checks.

  1. the label site alone: uniforms bit for bit, probabilities within 1e-4, EVERY row's class, pixel columns untouched, and the
     same rows inside a four times larger call giving identical bits;
  2. the CD step with labels against the same chain run through the public calls (half steps, the label site, the statistics
     hook), k = 1, k = 2 and a persistent chain; `which` masks, the momentum route, the epoch call against a step loop;
  3. one anchored step against the restatement's full step;
  4. class logits and posteriors against the restatement, pixels alone and with a label block behind them, an overflow row;
  5. the host classes: a three-step fit(V, y) trajectory with a remainder batch, predict_proba, sample(label=), the refusals, a
     checkpoint round trip, a two-layer DBN with a label RBM on top;
  6. a learning check on four prototype classes.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # labels_ref.py lives beside this file
import labels_ref as R

pytestmark = pytest.mark.gpu

LR = 1e-3


def _engine(dev, W, b_h, b_v):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    return DeviceRBM(W, b_h, b_v, dev)


def _dm(x, dev):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    return DeviceMatrix.from_host(np.ascontiguousarray(x, dtype=np.float32), dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _unpack(delta, nv, nh):
    d = delta.cpu().numpy().astype(np.float64)
    return d[:nv * nh].reshape(nv, nh), d[nv * nh:nv * nh + nh], d[nv * nh + nh:]


# ---- 1. the label site ---------------------------------------------------------------------------------------------------------
ALL_SITE_SHAPES = R.SITE_SHAPES + R.LOOP_SHAPES      # (the second list: n_hid >= 128, the two-block main loop of the kernel)


@pytest.mark.parametrize("shape", ALL_SITE_SHAPES, ids=["x".join(map(str, s)) for s in ALL_SITE_SHAPES])
def test_label_site(gpu_device, shape):
    rows, n_pix, C, n_hid = shape
    W, b_v, h = R.site_inputs(*shape)
    p_ref, u_ref, cls_ref, margin = R.label_site(W, b_v, h, n_pix, R.SITE_SEED, R.SITE_STREAM, R.SITE_STEP)
    e = _engine(gpu_device, W, np.zeros(n_hid, np.float32), b_v)
    # v: real-valued pixels and a block of garbage that the site must replace
    v0 = np.random.default_rng(8).normal(0, 1, (rows, n_pix + C)).astype(np.float32)
    v = _dm(v0, gpu_device)
    out = e.label_sample(_dm(h, gpu_device), v, C, R.SITE_SEED, R.SITE_STREAM, R.SITE_STEP, want_prob=True, want_u=True)
    torch.cuda.synchronize()
    u, p, got = out["u"].cpu().numpy(), out["prob"].to_numpy(), v.to_numpy()
    assert np.array_equal(u.view(np.uint32), u_ref.view(np.uint32)), "uniforms differ from the Philox contract"
    err = float(np.max(np.abs(p - p_ref)))
    print("%s: max |p - p_ref| = %.3g, nearest |u - boundary| = %.3g" % (shape, err, margin.min()))
    assert err <= R.TOL_P
    assert np.array_equal(got[:, n_pix:].argmax(axis=1), cls_ref), "rows %s drew another class" % np.nonzero(got[:, n_pix:].argmax(axis=1) != cls_ref)[0]
    assert np.array_equal(got[:, n_pix:], R.one_hot(cls_ref, C))
    assert np.array_equal(got[:, :n_pix].view(np.uint32), v0[:, :n_pix].view(np.uint32)), "pixel columns were written"
    # the same rows inside a four times larger call: identical bits
    h4 = np.concatenate([h, (np.random.default_rng(4).random((3 * rows, n_hid)) < .5).astype(np.float32)])
    v4 = _dm(np.concatenate([v0, np.zeros((3 * rows, n_pix + C), np.float32)]), gpu_device)
    out4 = e.label_sample(_dm(h4, gpu_device), v4, C, R.SITE_SEED, R.SITE_STREAM, R.SITE_STEP, want_prob=True, want_u=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out4["prob"].view()[:rows]), _bits(out["prob"].view()))
    assert torch.equal(_bits(out4["u"][:rows]), _bits(out["u"])) and torch.equal(_bits(v4.view()[:rows]), _bits(v.view()))
    # the promises of the argument checks
    from keras_unsupervised_amd import _lib
    for bad in (1, 65, n_pix + C):
        with pytest.raises(_lib.KurbmError, match="kurbm error -1"):
            e.label_sample(_dm(h, gpu_device), v, bad, 1, 1, 1)


# ---- 2. the step against the same chain through the public calls -----------------------------------------------------------
def _public_chain(e, Vd, rows, C, seed, step, k, chain_start, dev):
    """The chain of kurbm_cd_step_labels out of public calls; returns (dW tensor, db_h, db_v float64, v_neg DeviceMatrix,
    abs_dW, abs_db_h)."""
    from keras_unsupervised_amd import _lib
    S, B, N = _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, _lib.NOISE_NONE
    h_pos = e.half_step("vh", Vd, rows, 0, S, B, seed, 0, step)["sample"]
    h = h_pos if chain_start is None else e.half_step("vh", chain_start, rows, 0, S, B, seed, 32, step)["sample"]
    v = None
    for t in range(1, k + 1):
        v = e.half_step("hv", h, rows, 0, S, B, seed, 2 * t - 1, step)["sample"]
        e.label_sample(h, v, C, seed, 2 * t - 1, step)
        if t < k:
            h = e.half_step("vh", v, rows, 0, S, B, seed, 2 * t, step)["sample"]
    h_neg = e.half_step("vh", v, rows, 0, S, N, 0, 0, 0, want_sample=False, want_prob=True)["prob"]
    dW = e.outer_delta(Vd, h_pos, v, h_neg, rows)
    torch.cuda.synchronize()
    vp, hp, vn, hn = (m.to_numpy().astype(np.float64) for m in (Vd, h_pos, v, h_neg))
    return (dW.cpu().numpy().astype(np.float64), hp.sum(axis=0) - hn.sum(axis=0), vp.sum(axis=0) - vn.sum(axis=0), v,
            vp.T @ hp + vn.T @ hn, hp.sum(axis=0) + hn.sum(axis=0))


@pytest.mark.parametrize("rows", [200, 64])
@pytest.mark.parametrize("k,pcd", [(1, False), (2, False), (1, True), (2, True)], ids=["k1", "k2", "k1-chain", "k2-chain"])
def test_step_equals_the_public_chain(gpu_device, rows, k, pcd):
    n_pix, C, n_hid = 37, 10, 52
    nv = n_pix + C
    W, b_h, b_v = R.model(n_pix, C, n_hid)
    V, _ = R.labelled_batch(rows, n_pix, C)
    chain0, _ = R.labelled_batch(rows, n_pix, C, seed=6)
    e = _engine(gpu_device, W, b_h, b_v)
    Vd = _dm(V, gpu_device)
    chain = _dm(chain0, gpu_device) if pcd else None
    e.cd_step(Vd, rows, 0, LR, 42, 3, k=k, apply=False, emit_delta=True, v_chain=chain, n_labels=C)
    torch.cuda.synchronize()
    dW, db_h, db_v = _unpack(e.delta, nv, n_hid)
    assert np.array_equal(e.get_weights()[0], W), "apply = 0 wrote the weights"
    rW, rb_h, rb_v, v_neg, aW, ab_h = _public_chain(e, Vd, rows, C, 42, 3, k, _dm(chain0, gpu_device) if pcd else None, gpu_device)
    print("rows %d k %d chain %s: max |dW - ref| / bound = %.3g, |db_h - ref| / bound = %.3g"
          % (rows, k, pcd, np.max(np.abs(dW - rW) / (R.TOL_GEMM * np.maximum(aW, 1))), np.max(np.abs(db_h - rb_h) / (R.TOL_GEMM * np.maximum(ab_h, 1)))))
    assert np.all(np.abs(dW - rW) <= R.TOL_GEMM * np.maximum(aW, 1.0))
    assert np.all(np.abs(db_h - rb_h) <= R.TOL_GEMM * np.maximum(ab_h, 1.0))
    assert np.array_equal(db_v[n_pix:], rb_v[n_pix:]), "label entries of db_v: %s vs %s" % (db_v[n_pix:], rb_v[n_pix:])
    assert np.array_equal(db_v[:n_pix], rb_v[:n_pix]) and db_v[n_pix:].sum() == 0.0
    if pcd:
        got = chain.to_numpy()
        assert np.array_equal(got, v_neg.to_numpy()), "the persistent chain is not the chain's last visibles"
        blk = got[:, n_pix:]
        assert set(np.unique(blk)) <= {0.0, 1.0} and np.array_equal(blk.sum(axis=1), np.ones(rows)), "a block of the chain is not one-hot"


def test_which_masks_momentum_route_and_epoch(gpu_device):
    from keras_unsupervised_amd import _lib
    n_pix, C, n_hid, rows = 37, 10, 52, 64
    nv = n_pix + C
    W, b_h, b_v = R.model(n_pix, C, n_hid)
    V, _ = R.labelled_batch(150, n_pix, C)
    Vd = _dm(V, gpu_device)
    ref = _engine(gpu_device, W, b_h, b_v)
    ref.cd_step(Vd, rows, 0, LR, 42, 3, emit_delta=True, n_labels=C)          # apply + emit: all three variables
    full = ref.get_weights()
    for which in (1, 2, 4, 6):
        e = _engine(gpu_device, W, b_h, b_v)
        e.cd_step(Vd, rows, 0, LR, 42, 3, which=which, n_labels=C)
        got = e.get_weights()
        for i, (bit, x0) in enumerate(((1, W), (2, b_h), (4, b_v))):
            assert np.array_equal(got[i], full[i] if which & bit else x0), "which = %d, variable %d" % (which, i)
    # the momentum route: the same launch sequence, the update through the velocity == apply_delta_mom of the emitted delta
    mu, lam = 0.9, 1e-3
    a, b = _engine(gpu_device, W, b_h, b_v), _engine(gpu_device, W, b_h, b_v)
    a.cd_step(Vd, rows, 0, LR, 42, 3, emit_delta=True, momentum=(mu, lam), n_labels=C)
    assert torch.equal(a.delta, ref.delta), "the momentum step emits another delta"
    b.apply_delta(LR, delta=ref.delta, momentum=(mu, lam))
    torch.cuda.synchronize()
    g = _unpack(ref.delta, nv, n_hid)
    for i, (pa, pb, p0) in enumerate(zip(a.get_weights(), b.get_weights(), (W, b_h, b_v))):
        tol = 2.0 ** -21 * (np.abs(LR * g[i]) + np.abs(LR * lam * p0)) + 2.0 ** -23 * np.abs(p0)
        assert np.all(np.abs(pa.astype(np.float64) - pb) <= tol), "momentum route, variable %d" % i
        assert not np.array_equal(pa, p0)
    for va, vb in zip(a.get_velocity(), b.get_velocity()):
        assert np.allclose(va, vb, rtol=2.0 ** -20, atol=1e-12)
    with pytest.raises(_lib.KurbmError, match="kurbm error -1"):       # the momentum entry points apply in place
        a.cd_step(Vd, rows, 0, LR, 42, 3, apply=False, emit_delta=True, momentum=(mu, lam), n_labels=C)
    # the epoch call == a step loop, bit for bit (two full batches and a remainder of 22)
    ep, lp = _engine(gpu_device, W, b_h, b_v), _engine(gpu_device, W, b_h, b_v)
    assert ep.cd_epoch(Vd, 150, rows, LR, 42, 5, n_labels=C) == 3
    for i, lo in enumerate(range(0, 150, rows)):
        lp.cd_step(Vd, min(rows, 150 - lo), lo, LR, 42, 5 + i, n_labels=C)
    for x, y in zip(ep.get_weights(), lp.get_weights()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # Gaussian visibles and a bad label count are refused
    from keras_unsupervised_amd.ebm.engine import MODE_VISIBLE_GAUSSIAN
    for kw in (dict(mode=MODE_VISIBLE_GAUSSIAN, n_labels=C), dict(n_labels=1), dict(n_labels=nv)):
        with pytest.raises(_lib.KurbmError, match="kurbm error -1"):
            ep.cd_step(Vd, rows, 0, LR, 42, 3, **kw)


# ---- 3. one anchored step ------------------------------------------------------------------------------------------------------
def test_anchored_step(gpu_device):
    rows, n_pix, C, n_hid = R.ANCHOR
    nv = n_pix + C
    W, b_h, b_v = R.model(n_pix, C, n_hid)
    V, _ = R.labelled_batch(rows, n_pix, C)
    s = R.cd_step(W, b_h, b_v, V, C, R.ANCHOR_SEED, R.ANCHOR_STEP)
    e = _engine(gpu_device, W, b_h, b_v)
    e.cd_step(_dm(V, gpu_device), rows, 0, LR, R.ANCHOR_SEED, R.ANCHOR_STEP, apply=False, emit_delta=True, n_labels=C)
    torch.cuda.synchronize()
    for name, got, want in zip(("dW", "db_h", "db_v"), _unpack(e.delta, nv, n_hid), (s["dW"], s["db_h"], s["db_v"])):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print("%s: worst |d - d_ref| / max(1, |d_ref|) = %.3g" % (name, err.max()))
        assert err.max() <= R.TOL_STEP, name


# ---- 4. class logits ---------------------------------------------------------------------------------------------------------
LOGIT_SHAPES = R.SITE_SHAPES + [(5, 37, 10, 52)]


@pytest.mark.parametrize("wide", [False, True], ids=["pixels", "pixels+block"])
@pytest.mark.parametrize("shape", LOGIT_SHAPES, ids=["x".join(map(str, s)) for s in LOGIT_SHAPES])
def test_class_logits(gpu_device, shape, wide):
    rows, n_pix, C, n_hid = shape
    W, b_v, _ = R.site_inputs(*shape)
    b_h = np.random.default_rng(32).normal(0, .3, n_hid).astype(np.float32)
    g = np.random.default_rng(6)
    v = g.normal(0, 1, (rows, n_pix)).astype(np.float32)
    v[0] = 100.0 * np.sign(W[:n_pix, 0])                    # an overflow row: pre-activation 0 far beyond 88
    assert float(v[0].astype(np.float64) @ W[:n_pix, 0] + b_h[0]) > 88.0
    if wide:
        v = np.concatenate([v, g.normal(0, 1, (rows, C)).astype(np.float32)], axis=1)      # a "block" of garbage: ignored
    want, mag = R.class_logits(W, b_h, b_v, v, n_pix)
    p_want = R.posterior(want)
    e = _engine(gpu_device, W, b_h, b_v)
    logits, prob = e.class_logits(_dm(v, gpu_device), C)
    torch.cuda.synchronize()
    lg, pr = logits.to_numpy().astype(np.float64), prob.to_numpy().astype(np.float64)
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(pr))
    bound = R.TOL_GEMM * mag
    print("%s: worst |logit - ref| / bound = %.3g, worst |p - ref| / bound = %.3g"
          % (shape, np.max(np.abs(lg - want) / bound), np.max(np.abs(pr - p_want) / bound.max(axis=1, keepdims=True))))
    assert np.all(np.abs(lg - want) <= bound)
    assert np.all(np.abs(pr - p_want) <= bound.max(axis=1, keepdims=True))
    assert np.max(np.abs(pr.sum(axis=1) - 1.0)) <= 1e-5
    # rows do not depend on their neighbours: the first rows alone give the same bits
    few = min(rows, 3)
    l2, p2 = e.class_logits(_dm(v[:few], gpu_device), C)
    assert torch.equal(_bits(l2.view()), _bits(logits.view()[:few])) and torch.equal(_bits(p2.view()), _bits(prob.view()[:few]))


# ---- 5. the host classes -----------------------------------------------------------------------------------------------------
def _fit_problem():
    N, n_pix, C, n_hid = R.FIT_SHAPE
    W, b_h, b_v = R.model(n_pix, C, n_hid, std=.1)
    V, y = R.labelled_batch(N, n_pix, C)
    return N, n_pix, C, n_hid, W, b_h, b_v, V, y


def _rbm(W, b_h, b_v, C, epochs=1, **kw):
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM
    return RBM({"batch_size": R.FIT_BATCH, "epochs": epochs, "lr": R.FIT_LR}, W.shape[1], mode=MODE_VISIBLE_BERNOULLI, seed=R.FIT_SEED,
               weights=(W, b_h, b_v), device="cuda:0", n_labels=C, **kw)


def test_fit_trajectory(gpu_device, capsys):
    """Three steps (64, 64 and a remainder of 22 rows) of fit(V, y) against the restatement: (param - param_0) / lr, the summed
    updates, within 1e-4 max(1, |ref|)."""
    N, n_pix, C, n_hid, W, b_h, b_v, V, y = _fit_problem()
    ref = R.fit(W, b_h, b_v, V, C, R.FIT_BATCH, 1, R.FIT_LR, R.FIT_SEED)
    rbm = _rbm(W, b_h, b_v, C, compute_dtype="auto")
    assert rbm._compute() == "fp32"
    rbm.fit(V[:, :n_pix], verbose=0, y=y)
    assert rbm._update_count == 3
    for name, got, want, x0 in zip(("W", "b_h", "b_v"), rbm.get_weights(), ref[:3], (W, b_h, b_v)):
        d, d_ref = (got.astype(np.float64) - x0) / R.FIT_LR, (want - x0) / R.FIT_LR
        err = np.abs(d - d_ref) / np.maximum(1.0, np.abs(d_ref))
        print("%s: worst error / max(1, |ref|) = %.3g" % (name, err.max()))
        assert err.max() <= R.TOL_STEP, name
    # the joined matrix without y is the same fit; the step loop with the score pass (verbose = 1) gives the same bits
    for kw, data in ((dict(verbose=0), (rbm.join(V[:, :n_pix], y),)), (dict(verbose=1, y=y), (V[:, :n_pix],))):
        twin = _rbm(W, b_h, b_v, C)
        twin.fit(*data, **kw)
        for a, b in zip(twin.get_weights(), rbm.get_weights()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(twin.last_scores) == 3 and np.all(np.isfinite(twin.last_scores))
    capsys.readouterr()


def test_predict_sample_refusals_and_checkpoint(gpu_device, tmp_path):
    from keras_unsupervised_amd.ebm import checkpoint
    N, n_pix, C, n_hid, W, b_h, b_v, V, y = _fit_problem()
    rbm = _rbm(W, b_h, b_v, C, persistent=True)
    rbm.fit(V, verbose=0)                                     # the joined layout; a persistent chain
    blk = rbm.full_chain()[:, n_pix:]
    assert np.array_equal(blk.sum(axis=1), np.ones(R.FIT_BATCH)) and set(np.unique(blk)) <= {0.0, 1.0}
    Wn, bhn, bvn = rbm.get_weights()
    p = rbm.predict_proba(V[:, :n_pix])
    assert p.shape == (N, C) and np.max(np.abs(p.sum(axis=1) - 1.0)) <= 1e-5
    assert np.max(np.abs(p - R.posterior(R.class_logits(Wn, bhn, bvn, V, n_pix)[0]))) <= R.TOL_P
    assert np.array_equal(rbm.predict_proba(V), p) and np.array_equal(rbm.predict(V), p.argmax(axis=1))
    lg = rbm.class_logits(torch.from_numpy(V[:, :n_pix]))
    assert isinstance(lg, torch.Tensor) and lg.shape == (N, C)
    # class-conditional samples keep the clamped block
    s = rbm.sample(8, burn_in=3, label=4)
    assert s.shape == (8, n_pix + C) and np.array_equal(s[:, n_pix:], R.one_hot([4] * 8, C)) and set(np.unique(s)) <= {0.0, 1.0}
    labels = np.arange(8) % C
    s = rbm.gibbs(V[:8, :n_pix], n_steps=2, label=labels)
    assert np.array_equal(s[:, n_pix:], R.one_hot(labels, C))
    # inv_transform draws its block through the label site: one-hot rows
    v = rbm.inv_transform(rbm.transform(V)[0])[0]
    assert v.shape == (N, n_pix + C) and np.array_equal(v[:, n_pix:].sum(axis=1), np.ones(N)) and set(np.unique(v)) <= {0.0, 1.0}
    # the refusals
    for call in (lambda: rbm.sample(4, burn_in=1), lambda: rbm.gibbs(V[:4]), lambda: rbm.log_partition(),
                 lambda: rbm.log_likelihood(V), lambda: rbm.fit(np.ones_like(V), verbose=0),
                 lambda: rbm.fit(V, verbose=0, y=y), lambda: rbm.predict(V[:, :5])):
        with pytest.raises(ValueError):
            call()
    # checkpoint round trip
    stem = str(tmp_path / "label_rbm")
    checkpoint.save_rbm(rbm, stem)
    back = checkpoint.load_rbm(stem, device="cuda:0")
    assert back.n_labels == C and back.get_config() == rbm.get_config() and back._update_count == rbm._update_count
    assert np.array_equal(back.predict_proba(V), p) and np.array_equal(back.full_chain(), rbm.full_chain())


def test_dbn_with_a_label_rbm_on_top(gpu_device, capsys):
    from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, RBM
    X, y = R.prototypes_data(n_rows=64, n_pix=12, C=3, seed=2)
    hps = {"batch_size": 32, "epochs": 2, "lr": 0.01}
    dbn = DBN()
    dbn.add_stack(RBM(hps, 8, name="bottom", mode=MODE_VISIBLE_BERNOULLI, seed=1, device="cuda:0"))
    dbn.add_stack(RBM(hps, 6, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=2, device="cuda:0", n_labels=3))
    dbn.fit(X, verbose=0, y=y)
    top = dbn._layers()[1]
    assert top.built and top.input_shape == (None, 11) and top._update_count == 4
    p = dbn.predict_proba(X)
    assert p.shape == (64, 3) and np.max(np.abs(p.sum(axis=1) - 1.0)) <= 1e-5
    yp = dbn.predict(X)
    assert yp.shape == (64,) and yp.min() >= 0 and yp.max() < 3 and np.array_equal(yp, p.argmax(axis=1))
    s = dbn.sample(4, burn_in=2, label=1)
    assert s.shape == (4, 12) and set(np.unique(s)) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        dbn.sample(4, burn_in=2)
    with pytest.raises(ValueError):
        dbn.fit(X, verbose=0)
    capsys.readouterr()


# ---- 6. learning ---------------------------------------------------------------------------------------------------------------
def test_learns_the_prototypes(gpu_device):
    """Four prototype classes, 32 pixels, 5 % flips, 512 rows, 32 hidden units, 10 epochs of batch 64 at lr 0.01: the accuracy of
    predict() on the training set must reach the restatement-trained model's minus 0.05 (the two runs share every seed; the margin
    covers draws inside the fp32 rounding band that let them diverge).  The restatement's accuracy is 1.0000 (chance: 0.25)."""
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM
    L = R.LEARN
    X, y = R.prototypes_data()
    W, b_h, b_v = R.learn_init()
    ref = R.fit(W, b_h, b_v, np.concatenate([X, R.one_hot(y, L["C"])], axis=1), L["C"], L["batch"], L["epochs"], L["lr"], L["seed"])
    acc_ref = float((R.predict(ref[0], ref[1], ref[2], X, L["n_pix"]) == y).mean())
    assert acc_ref >= 2.0 / L["C"]
    rbm = RBM({"batch_size": L["batch"], "epochs": L["epochs"], "lr": L["lr"]}, L["n_hid"], mode=MODE_VISIBLE_BERNOULLI, seed=L["seed"],
              weights=(W, b_h, b_v), device="cuda:0", n_labels=L["C"])
    rbm.fit(X, verbose=0, y=y)
    acc = float((rbm.predict(X) == y).mean())
    print("accuracy %.4f (restatement %.4f)" % (acc, acc_ref))
    assert acc >= acc_ref - 0.05
