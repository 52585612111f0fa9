"""GPU tier of DBN fine-tuning (include/kurbm.h: kurbm_backprop_delta, kurbm_backprop_layer, kurbm_disc_backprop;
csrc/kurbm_backprop.hip; DBN.fine_tune) against the float64 restatement of tests/backprop_ref.py, whose own standing the CPU tier
(tests/test_backprop_host.py) checks against central differences and torch.autograd.

  1. the site alone: delta within 1e-6 max(1, |e|) (relu and linear: exact), db_h at 4 x the restatement's own fp32 noise +
     TOL_GEMM abs_db_h; wide leading dimensions with NaN padding, in place and out of place; the first rows alone give the same
     bits; two calls give the same bits;
  2. a layer on the lattice (tests/lattice.py), linear site: e_in, dW, db_h are the float64 result's exact bits, db_v is zeros;
  3. a layer, sigmoid and relu, against the restatement at the bar of 1; e_in = NULL leaves the delta's bits alone;
  4. the top layer: delta and nll_mean bit for bit kurbm_class_grad's / kurbm_disc_step's; e_in against float64 products of the GPU's
     OWN plane g and against the restatement;
  5. fine_tune: one step = the hooks plus the applies, an epoch = the step loop, two runs -- all bit for bit; the trajectory
     against the restatement's loop; a one-layer DBN is RBM.fit(objective='discriminative');
  6. end to end on the prototype classes, and the checkpoint round trip;
  7. refusals, with nothing written.
"""
import ctypes as C_
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # backprop_ref.py and its neighbours live beside this file
import backprop_ref as B
import labels_ref as R
import lattice as L

pytestmark = pytest.mark.gpu

ACTS = [B.ACT_SIGMOID, B.ACT_RELU, B.ACT_LINEAR]
ACT_IDS = {B.ACT_SIGMOID: "sigmoid", B.ACT_RELU: "relu", B.ACT_LINEAR: "linear"}
# (rows, n_hid), row tiles of 16 rows and column slices of 256: a ragged last row tile and fewer columns than one slice; an odd ragged
# slice (137 = 34 groups of four and one column); a second slice that is nearly empty (one group)
SITE_SHAPES = [(37, 36), (200, 137), (130, 260)]
# (rows, n_in, n_out)
LAYER_SHAPES = [(37, 70, 36), (200, 330, 137), (130, 300, 260)]
IDS = lambda shapes: ["x".join(map(str, s)) for s in shapes]
ERR_ARG, ERR_WS = -1, -4


def _engine(dev, W, b_h, b_v):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    return DeviceRBM(np.array(W), np.array(b_h), np.array(b_v), dev)      # (copies: the fixtures are read-only)


def _dm(x, dev, pad=0, fill=float("nan")):
    """DeviceMatrix of host array x; pad > 0: a leading dimension `pad` floats beyond round_up(cols, 4), the padding `fill`."""
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix, round_up
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not pad:
        return DeviceMatrix.from_host(x.copy(), dev)
    rows, cols = x.shape
    ld = round_up(cols, 4) + pad
    t = torch.full((rows, ld), fill, dtype=torch.float32, device=dev)
    t[:, :cols].copy_(torch.from_numpy(x))
    return DeviceMatrix(t, rows, cols, ld)


def _nan_plane(rows, cols, dev, pad=8):
    return _dm(np.full((rows, cols), np.nan, np.float32), dev, pad)


def _pad_is_nan(m):
    return m.ld == m.cols or bool(torch.isnan(m.t[:m.rows, m.cols:]).all().item())


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _unpack(delta, nv, nh):
    d = delta.cpu().numpy()
    return d[:nv * nh].reshape(nv, nh), d[nv * nh:nv * nh + nh], d[nv * nh + nh:]


def _held(name, got, ref, ref32, mag):
    """The bar of tests/test_gpu_classgrad.py: 4 x the restatement's own fp32 noise at this fixture + TOL_GEMM x the un-cancelled magnitude."""
    noise = float(np.abs(ref32.astype(np.float64) - ref).max())
    bar = 4 * noise + R.TOL_GEMM * mag
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: numpy-fp32 noise %.3g, worst error %.3g, worst error / bar %.3g" % (name, noise, float(err.max()), float((err / np.maximum(bar, 1e-30)).max())))
    assert np.isfinite(got).all() and np.all(err <= bar), name


# ---- 1. the site alone ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _site_fixture(shape, act):
    rows, n_hid = shape
    g = np.random.default_rng(5100 + rows + act)
    e = g.normal(0, 1, (rows, n_hid)).astype(np.float32)
    pre = g.normal(0, 1.5, (rows, n_hid))
    x = B.activate(pre, act).astype(np.float32)           # sigmoid: (0, 1); relu: exact zeros and positives; linear: not read
    ref = B.site(e.astype(np.float64), x.astype(np.float64), act)
    ref32 = B.site(e, x, act)
    for a in (e, x, ref, ref32):
        a.setflags(write=False)
    return e, x, ref, ref32


def _site_call(eng, e, x, act, delta, rows=None, ws=None):
    rows = e.rows if rows is None else rows
    ws = eng.backprop_workspace(rows, 1) if ws is None else ws
    db_h = torch.full((eng.n_hid,), float("nan"), dtype=torch.float32, device=eng.device)
    from keras_unsupervised_amd._lib import check
    check(eng.lib.kurbm_backprop_delta(eng.ctx.handle, e.ptr(), e.ld, x.ptr(), x.ld, rows, eng.n_hid, act, delta.ptr(), delta.ld,
                                       db_h.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream()))
    torch.cuda.synchronize()
    return db_h.cpu().numpy()


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("act", ACTS, ids=[ACT_IDS[a] for a in ACTS])
@pytest.mark.parametrize("shape", SITE_SHAPES, ids=IDS(SITE_SHAPES))
def test_site_against_the_restatement(gpu_device, shape, act, in_place):
    rows, n_hid = shape
    e, x, ref, ref32 = _site_fixture(shape, act)
    eng = _engine(gpu_device, np.zeros((4, n_hid), np.float32), np.zeros(n_hid, np.float32), np.zeros(4, np.float32))
    ed, xd = _dm(e, gpu_device, pad=8), _dm(x, gpu_device, pad=12)
    dd = ed if in_place else _nan_plane(rows, n_hid, gpu_device, pad=4)
    db_h = _site_call(eng, ed, xd, act, dd)
    delta = dd.to_numpy()
    assert np.isfinite(delta).all() and np.isfinite(db_h).all(), "a padding NaN reached a result"
    assert _pad_is_nan(ed) and _pad_is_nan(xd) and _pad_is_nan(dd), "padding columns were written"
    if not in_place:
        assert _same(ed.to_numpy(), e), "e was written by an out-of-place call"
    assert _same(xd.to_numpy(), x)
    err = np.abs(delta.astype(np.float64) - ref)
    print("%s %s: worst |delta - ref| / max(1, |e|) = %.3g" % (shape, ACT_IDS[act], float((err / np.maximum(1.0, np.abs(e))).max())))
    assert np.all(err <= 1e-6 * np.maximum(1.0, np.abs(e)))
    if act == B.ACT_RELU:
        assert _same(delta, np.where(x > 0, e, np.float32(0)))            # a select: exact where x_out is given
    if act == B.ACT_LINEAR:
        assert _same(delta, e)
    _held("db_h", db_h, ref.sum(axis=0), ref32.sum(axis=0, dtype=np.float32), np.abs(ref).sum(axis=0))
    # the same call again: the same bits (in place, e has to be put back first)
    e2 = _dm(e, gpu_device, pad=8)
    d2 = e2 if in_place else _nan_plane(rows, n_hid, gpu_device, pad=4)
    db_h2 = _site_call(eng, e2, xd, act, d2)
    assert _same(d2.to_numpy(), delta) and _same(db_h2, db_h)
    # the first 5 rows alone: a row's delta does not depend on how many rows share the launch
    e5 = _dm(e[:5], gpu_device, pad=8)
    d5 = e5 if in_place else _nan_plane(5, n_hid, gpu_device, pad=4)
    _site_call(eng, e5, _dm(x[:5], gpu_device, pad=12), act, d5)
    assert _same(d5.to_numpy(), delta[:5])
    # ... and the engine's method is this call
    dm2, dbh2 = eng.backprop_delta(_dm(e, gpu_device), _dm(x, gpu_device), act)
    torch.cuda.synchronize()
    assert _same(dm2.to_numpy(), delta) and _same(dbh2.cpu().numpy(), db_h)


# ---- 2. a layer on the lattice -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "mid"])
def test_linear_layer_is_exact_on_the_lattice(gpu_device, shape):
    rows, n_in, n_out = L.SHAPES[shape]
    Wi, eb = L.weights("dense", n_in, n_out)                            # |m| < 2^11 at 2^-10
    g = np.random.default_rng(5200)
    ei = L._odd(g, 1, 8, (rows, n_out)) * L._signs(g, (rows, n_out))    # dense odd numerators in [-7, 7] at 2^-3
    xi, ex, _ = L.data("b8n", rows, n_in)                               # dense 1 .. 15 at 2^-4
    fx_ein = L.Fixture("backprop e_in", ei, -3, Wi.T, eb, np.zeros(n_in, np.int64))
    fx_dw = L.Fixture("backprop dW", xi.T, ex, ei, -3, np.zeros(n_out, np.int64))
    fx_dbh = L.Fixture("backprop db_h", np.ones((1, rows), np.int64), 0, ei, -3, np.zeros(n_out, np.int64))
    for fx in (fx_ein, fx_dw, fx_dbh):
        L.certify(fx)
    L.coverage([fx_ein]), L.coverage([fx_dw])
    W = fx_ein.b.T.copy()
    eng = _engine(gpu_device, W, np.zeros(n_out, np.float32), np.zeros(n_in, np.float32))
    x_in, e = _dm(fx_dw.a.T.copy(), gpu_device, pad=8), _dm(fx_ein.a, gpu_device, pad=12)
    x_out = _nan_plane(rows, n_out, gpu_device)                         # the linear site does not read it
    e_in = _nan_plane(rows, n_in, gpu_device, pad=4)
    eng.delta_buffer().fill_(float("nan"))
    delta = eng.backprop_layer(B.ACT_LINEAR, x_in, x_out, e, e_in=e_in)
    torch.cuda.synchronize()
    dW, db_h, db_v = _unpack(delta, n_in, n_out)
    assert _same(e_in.to_numpy(), fx_ein.ref()), "e_in = e.W^T"
    assert _same(dW, fx_dw.ref()), "dW = x_in^T.e"
    assert _same(db_h, fx_dbh.ref()[0]), "db_h = sum e"
    assert np.array_equal(db_v.view(np.uint32), np.zeros(n_in, np.uint32)), "db_v"
    assert _same(e.to_numpy(), fx_ein.a), "delta = e"
    assert _pad_is_nan(x_in) and _pad_is_nan(e) and _pad_is_nan(e_in) and bool(torch.isnan(x_out.t).all().item())


# ---- 3. a layer against the restatement ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_fixture(shape, act):
    rows, n_in, n_out = shape
    g = np.random.default_rng(5300 + rows + act)
    W = g.normal(0, .1, (n_in, n_out)).astype(np.float32)
    b_h = g.normal(0, .3, n_out).astype(np.float32)
    x_in = (g.random((rows, n_in)) < .5).astype(np.float32)
    x_out = B.activate(x_in.astype(np.float64) @ W + b_h, act).astype(np.float32)
    e = g.normal(0, 1, (rows, n_out)).astype(np.float32)
    ref, ref32 = B.layer_backward(W, act, x_in, x_out, e), B.layer_backward(W, act, x_in, x_out, e, dt=np.float32)
    for a in (W, b_h, x_in, x_out, e, *ref.values(), *ref32.values()):
        a.setflags(write=False)
    return W, b_h, x_in, x_out, e, ref, ref32


@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=IDS(LAYER_SHAPES))
def test_layer_against_the_restatement(gpu_device, shape, act):
    rows, n_in, n_out = shape
    W, b_h, x_in, x_out, e, ref, ref32 = _layer_fixture(shape, act)
    eng = _engine(gpu_device, W, b_h, np.zeros(n_in, np.float32))
    xi, xo, ed = _dm(x_in, gpu_device, pad=8), _dm(x_out, gpu_device, pad=12), _dm(e, gpu_device, pad=4)
    e_in = _nan_plane(rows, n_in, gpu_device)
    eng.delta_buffer().fill_(float("nan"))
    delta = eng.backprop_layer(act, xi, xo, ed, e_in=e_in).clone()
    torch.cuda.synchronize()
    dW, db_h, db_v = _unpack(delta, n_in, n_out)
    d = ed.to_numpy()
    assert np.all(np.abs(d.astype(np.float64) - ref["delta"]) <= 1e-6 * np.maximum(1.0, np.abs(e)))
    _held("%s dW" % (shape,), dW, ref["dW"], ref32["dW"], ref["abs_dW"])
    _held("%s db_h" % (shape,), db_h, ref["db_h"], ref32["db_h"], ref["abs_db_h"])
    _held("%s e_in" % (shape,), e_in.to_numpy(), ref["e_in"], ref32["e_in"], ref["abs_e_in"])
    assert np.array_equal(db_v.view(np.uint32), np.zeros(n_in, np.uint32))
    assert _pad_is_nan(xi) and _pad_is_nan(xo) and _pad_is_nan(ed) and _pad_is_nan(e_in)
    assert _same(eng.get_weights()[0], W), "nothing is applied"
    # without e_in: the same delta, bit for bit
    ed2 = _dm(e, gpu_device, pad=4)
    eng.delta_buffer().fill_(float("nan"))
    bare = eng.backprop_layer(act, xi, xo, ed2)
    torch.cuda.synchronize()
    assert torch.equal(bare.view(torch.int32), delta.view(torch.int32)) and _same(ed2.to_numpy(), d)


# ---- 4. the top layer ----------------------------------------------------------------------------------------------------------
TOP_SHAPES = [(37, 70, 3, 36), (130, 300, 3, 200), (37, 70, 20, 36), (130, 300, 20, 200)]      # (rows, n_pix, C, n_hid)


@pytest.mark.parametrize("shape", TOP_SHAPES, ids=IDS(TOP_SHAPES))
def test_disc_backprop(gpu_device, shape):
    rows, n_pix, C, n_hid = shape
    W, b_h, b_v = R.model(n_pix, C, n_hid, std=.1)
    V, _ = R.labelled_batch(rows, n_pix, C)
    a, b, c = (_engine(gpu_device, W, b_h, b_v) for _ in range(3))
    vd = _dm(V, gpu_device, pad=8)
    hook = a.class_grad(vd, C)
    want_delta = hook["delta"].clone()
    want_nll = c.disc_step(_dm(V, gpu_device), rows, 0, 1e-3, C, want_nll=True)
    b.delta_buffer().fill_(float("nan"))
    delta, nll = b.disc_backprop(vd, C, want_nll=True)
    torch.cuda.synchronize()
    assert torch.equal(delta.view(torch.int32), want_delta.view(torch.int32)), "delta_out is kurbm_class_grad's"
    assert torch.equal(nll.view(torch.int32)[:1], want_nll.view(torch.int32)[:1]), "nll_mean is kurbm_disc_step's"
    e_in = _nan_plane(rows, n_pix, gpu_device, pad=4)
    b.delta_buffer().fill_(float("nan"))
    delta2, _ = b.disc_backprop(vd, C, e_in=e_in)
    torch.cuda.synchronize()
    assert torch.equal(delta2.view(torch.int32), want_delta.view(torch.int32)) and _pad_is_nan(e_in) and _pad_is_nan(vd)
    got = e_in.to_numpy()
    assert np.isfinite(got).all() and _same(b.get_weights()[0], W)
    # against float64 products of the GPU's OWN plane g = fl(S_y - H_bar): the rounding of the h -> v launch and nothing else
    g_gpu = (hook["S_y"].to_numpy() - hook["H_bar"].to_numpy()).astype(np.float64)
    Wp = W[:n_pix].astype(np.float64)
    err = np.abs(got - g_gpu @ Wp.T)
    mag = np.abs(g_gpu) @ np.abs(Wp).T
    print("%s: worst |e_in - g.W^T| / magnitude = %.3g" % (shape, float((err / np.maximum(mag, 1e-30)).max())))
    assert np.all(err <= R.TOL_GEMM * mag)
    # against the restatement: g is S_y - H_bar, each held to TOL_P by tests/test_gpu_classgrad.py, so e_in inherits 2 TOL_P sum_j |W_ij|
    ref = B.top_backward((W, b_h, b_v), C, V)
    err = np.abs(got - ref["e_in"])
    bar = 2 * R.TOL_P * np.abs(Wp).sum(axis=1)[None, :] + R.TOL_GEMM * ref["abs_e_in"]
    print("%s: worst |e_in - restatement| / bar = %.3g" % (shape, float((err / bar).max())))
    assert np.all(err <= bar)


# ---- 5. composition and trajectory ---------------------------------------------------------------------------------------------
def _dbn(lower, top, C, hps=None):
    from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, RBM
    T = B.TRAJ
    hps = hps or {"batch_size": T["batch"], "epochs": T["epochs"], "lr": T["lr"]}
    dbn = DBN()
    for i, (W, b_h, act) in enumerate(lower):
        mode = MODE_VISIBLE_GAUSSIAN if act == B.ACT_RELU else MODE_VISIBLE_BERNOULLI
        r = RBM(dict(hps), W.shape[1], name="l%d" % (i + 1), mode=mode, seed=i, device="cuda:0",
                weights=(np.array(W), np.array(b_h), np.zeros(W.shape[0], np.float32)))
        r.build((None, W.shape[0]))
        dbn.add_stack(r)
    t = RBM(dict(hps), top[0].shape[1], name="top", mode=MODE_VISIBLE_BERNOULLI, seed=9, device="cuda:0", n_labels=C,
            weights=tuple(np.array(x) for x in top))
    t.build((None, top[0].shape[0]))
    dbn.add_stack(t)
    return dbn


def _weights(dbn):
    return [w for layer in dbn._layers() for w in layer.get_weights()]


def _all_same(a, b):
    wa, wb = _weights(a), _weights(b)
    return len(wa) == len(wb) and all(_same(x, y) for x, y in zip(wa, wb))


@pytest.mark.parametrize("momentum", [None, (0.9, 1e-3)], ids=["plain", "momentum"])
@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
def test_one_step_is_the_hooks_plus_the_applies(gpu_device, act, momentum):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    T = B.TRAJ
    lower, top, V, y = B.traj_problem(act)
    rows, C, lr = T["batch"], T["C"], T["lr"]
    a, b = _dbn(lower, top, C), _dbn(lower, top, C)
    kw = dict(momentum=momentum[0], weight_decay=momentum[1]) if momentum else {}
    for step in range(2):        # (the second step reads the velocity the first one left)
        a.fine_tune(V[:rows], y[:rows], epochs=1, verbose=0, **kw)
        # by hand on b's engines: the existing half step and class_grad hook, the new entry points, the existing apply
        l1, l2, tp = (layer._dev for layer in b._layers())
        x0 = _dm(V[:rows], gpu_device)
        x1 = l1.half_step("vh", x0, rows, 0, act, 0, 0, 0, 0, want_sample=False, want_prob=True)["prob"]
        x2 = l2.half_step("vh", x1, rows, 0, act, 0, 0, 0, 0, want_sample=False, want_prob=True)["prob"]
        vt = _dm(np.concatenate([x2.to_numpy(), R.one_hot(y[:rows], C)], axis=1), gpu_device)
        d_top = tp.class_grad(vt, C, want_planes=False)["delta"].clone()
        e2 = DeviceMatrix.zeros(rows, l2.n_hid, gpu_device)
        tp.disc_backprop(vt, C, e_in=e2)
        e1 = DeviceMatrix.zeros(rows, l1.n_hid, gpu_device)
        d2 = l2.backprop_layer(act, x1, x2, e2, e_in=e1)
        d1 = l1.backprop_layer(act, x0, x1, e1)
        l1.apply_delta(lr, which=3, delta=d1, momentum=momentum)
        l2.apply_delta(lr, which=3, delta=d2, momentum=momentum)
        tp.apply_delta(lr, delta=d_top, momentum=momentum)
        torch.cuda.synchronize()
        assert _all_same(a, b), "step %d" % step
    assert not _same(_weights(a)[0], lower[0][0]) and np.isfinite(_weights(a)[0]).all()
    assert _same(_weights(a)[2], np.zeros(T["sizes"][0], np.float32)), "a lower layer's visible bias is left alone"
    assert [layer._update_count for layer in a._layers()] == [2, 2, 2]


@pytest.mark.parametrize("variant", ["plain", "momentum"])
@pytest.mark.parametrize("act", [B.ACT_SIGMOID, B.ACT_RELU], ids=["sigmoid", "relu"])
def test_epochs_are_the_step_loop_and_follow_the_float64_trajectory(gpu_device, act, variant, capsys):
    T = B.TRAJ
    lower, top, V, y = B.traj_problem(act)
    N, bs, C, lr = T["N"], T["batch"], T["C"], T["lr"]
    mom, decay = (T["momentum"], T["weight_decay"]) if variant == "momentum" else (0.0, 0.0)
    a, b, c = _dbn(lower, top, C), _dbn(lower, top, C), _dbn(lower, top, C)
    a.fine_tune(V, y, momentum=mom, weight_decay=decay, verbose=0)           # epochs, lr, batch size: the top layer's hps
    c.fine_tune(V, y, momentum=mom, weight_decay=decay, verbose=1)           # a second run, printing: the same bits
    for epoch in range(T["epochs"]):
        mu = mom[min(epoch, len(mom) - 1)] if isinstance(mom, list) else mom
        for lo in range(0, N, bs):
            b.fine_tune(V[lo:lo + bs], y[lo:lo + bs], epochs=1, lr=lr, batch_size=bs, momentum=mu, weight_decay=decay, verbose=0)
    torch.cuda.synchronize()
    assert _all_same(a, b), "an epoch is the step loop"
    assert _all_same(a, c), "two runs give the same bits"
    steps = T["epochs"] * 4
    assert [layer._update_count for layer in a._layers()] == [steps] * 3 and len(c.last_scores) == steps
    assert capsys.readouterr().out.count("score:") == steps
    # the first printed score is the restatement's mean nll at the initial weights (the bar of a row's nll: tests/test_gpu_classgrad.py)
    s0 = B.grad(lower, top, C, V[:bs], y[:bs])
    _, abs_terms = R.class_logits(top[0], top[1], top[2], s0["xs"][-1], T["sizes"][-1])
    assert abs(c.last_scores[0] - float(s0["nll"].mean())) <= 2 * R.TOL_GEMM * float(abs_terms.max()) + R.TOL_P
    # the float64 trajectory, at the project's bar on one (tests/test_gpu_labels.py): the summed updates (param - param_0) / lr
    rl, rt, rsteps, margin = B.fine_tune(lower, top, C, V, y, bs, T["epochs"], lr, momentum=mom, weight_decay=decay)
    assert rsteps == steps and (act != B.ACT_RELU or margin > B.RELU_MARGIN)
    got = _weights(a)
    want = [(rl[0][0], lower[0][0]), (rl[0][1], lower[0][1]), None, (rl[1][0], lower[1][0]), (rl[1][1], lower[1][1]), None,
            (rt[0], top[0]), (rt[1], top[1]), (rt[2], top[2])]
    names = ["W1", "b_h1", "b_v1", "W2", "b_h2", "b_v2", "W_top", "b_h_top", "b_v_top"]
    for name, g, w in zip(names, got, want):
        if w is None:
            assert not g.any(), name
            continue
        ref, x0 = w
        err = np.abs(g.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        d, d_ref = (g.astype(np.float64) - x0) / lr, (ref - x0) / lr
        err_d = np.abs(d - d_ref) / np.maximum(1.0, np.abs(d_ref))
        print("%s: worst parameter error / max(1, |ref|) = %.3g; of the summed updates = %.3g" % (name, err.max(), err_d.max()))
        assert err.max() <= R.TOL_STEP and err_d.max() <= R.TOL_STEP, name
        assert np.abs(d_ref).max() > 0, name


def test_one_layer_dbn_is_the_discriminative_fit(gpu_device):
    from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, RBM
    N, n_pix, C, n_hid = R.FIT_SHAPE
    W, b_h, b_v = R.model(n_pix, C, n_hid, std=.1)
    V, y = R.labelled_batch(N, n_pix, C)
    hps = {"batch_size": R.FIT_BATCH, "epochs": 2, "lr": R.FIT_LR}
    mk = lambda **kw: RBM(dict(hps), n_hid, mode=MODE_VISIBLE_BERNOULLI, seed=R.FIT_SEED, weights=(W, b_h, b_v), device="cuda:0", n_labels=C, **kw)
    rbm, top = mk(objective="discriminative"), mk()
    rbm.fit(V[:, :n_pix], y=y, verbose=0)
    top.build((None, n_pix + C))
    dbn = DBN()
    dbn.add_stack(top)
    dbn.fine_tune(V[:, :n_pix], y, verbose=0)
    for x, z, name in zip(rbm.get_weights(), top.get_weights(), ("W", "b_h", "b_v")):
        assert _same(x, z), name
    assert top._update_count == rbm._update_count == 6 and not _same(top.get_weights()[0], W)
    assert abs(dbn.class_log_likelihood(V[:, :n_pix], y) - rbm.class_log_likelihood(V[:, :n_pix], y)) == 0.0


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_pretrain_then_fine_tune_learns_and_checkpoints(gpu_device, tmp_path, capsys):
    from keras_unsupervised_amd.ebm import DBN, MODE_VISIBLE_BERNOULLI, RBM, checkpoint
    X, y = R.prototypes_data()
    hps = {"batch_size": 64, "epochs": 3, "lr": 0.01}
    dbn = DBN()
    dbn.add_stack(RBM(hps, 24, name="bottom", mode=MODE_VISIBLE_BERNOULLI, seed=1, device="cuda:0", compute_dtype="fp32"))
    dbn.add_stack(RBM(hps, 16, name="middle", mode=MODE_VISIBLE_BERNOULLI, seed=2, device="cuda:0", compute_dtype="fp32"))
    dbn.add_stack(RBM(hps, 16, name="top", mode=MODE_VISIBLE_BERNOULLI, seed=3, device="cuda:0", n_labels=4))
    dbn.fit(X, verbose=0, y=y)
    capsys.readouterr()
    w0 = [layer.rbm_weight.copy() for layer in dbn._layers()]
    counts = [layer._update_count for layer in dbn._layers()]
    ll0, acc0 = dbn.class_log_likelihood(X, y), float((dbn.predict(X) == y).mean())
    assert dbn.fine_tune(X, y, epochs=10, verbose=0) is None
    ll, acc = dbn.class_log_likelihood(X, y), float((dbn.predict(X) == y).mean())
    print("mean log p(y | v) %.4f -> %.4f, accuracy %.4f -> %.4f" % (ll0, ll, acc0, acc))
    assert ll > ll0 and acc >= acc0
    for layer, w in zip(dbn._layers(), w0):
        assert not _same(layer.rbm_weight, w) and np.isfinite(layer.rbm_weight).all(), layer.name
    assert [layer._update_count for layer in dbn._layers()] == [n + 80 for n in counts]
    # class_log_likelihood is the restatement's figure at the fine-tuned weights
    lower = [(l.rbm_weight, l.hidden_bias, B.ACT_SIGMOID) for l in dbn._layers()[:-1]]
    assert abs(ll - B.mean_log_posterior(lower, tuple(dbn._layers()[-1].get_weights()), 4, X, y)) <= R.TOL_P
    # the checkpoint round trip
    p = dbn.predict_proba(X)
    stem = str(tmp_path / "fine_tuned")
    checkpoint.save_dbn(dbn, stem)
    back = checkpoint.load_dbn(stem, device="cuda:0")
    assert _all_same(dbn, back) and np.array_equal(back.predict_proba(X), p)
    assert [layer._update_count for layer in back._layers()] == [layer._update_count for layer in dbn._layers()]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_device):
    rows, n_in, n_out, C = 37, 70, 36, 3
    W, b_h, x_in, x_out, e, _, _ = _layer_fixture((rows, n_in, n_out), B.ACT_SIGMOID)
    eng = _engine(gpu_device, W, b_h, np.zeros(n_in, np.float32))
    lib, ctx, P, st = eng.lib, eng.ctx.handle, C_.byref(eng.params), eng._stream()
    xi, xo, ed, ei = _dm(x_in, gpu_device), _dm(x_out, gpu_device), _dm(e, gpu_device), _dm(np.full((rows, n_in), 7.0), gpu_device)
    dd = _dm(np.full((rows, n_out), 7.0), gpu_device)
    db_h = torch.full((n_out,), 7.0, dtype=torch.float32, device=gpu_device)
    delta = eng.delta_buffer()
    delta.fill_(7.0)
    ws, ws1 = eng.backprop_workspace(rows), eng.backprop_workspace(rows, 1)
    assert lib.kurbm_backprop_workspace_bytes(ctx, 0, n_in, n_out) == 0 and lib.kurbm_backprop_workspace_bytes(ctx, rows, n_in, 0) == 0
    assert int(lib.kurbm_backprop_workspace_bytes(ctx, rows, n_in, n_out)) == ws.numel() > 16 and ws1.numel() > 16

    def site(**k):
        return lib.kurbm_backprop_delta(ctx, k.get("e", ed.ptr()), k.get("lde", ed.ld), k.get("x", xo.ptr()), k.get("ldx", xo.ld),
                                        k.get("rows", rows), n_out, k.get("act", 0), k.get("d", dd.ptr()), k.get("ldd", dd.ld),
                                        k.get("db_h", db_h.data_ptr()), k.get("ws", ws1.data_ptr()), k.get("n", ws1.numel()), st)

    def layer(**k):
        return lib.kurbm_backprop_layer(ctx, P, k.get("act", 0), k.get("xi", xi.ptr()), k.get("ldin", xi.ld), k.get("xo", xo.ptr()),
                                        k.get("ldout", xo.ld), k.get("e", ed.ptr()), k.get("lde", ed.ld), k.get("rows", rows),
                                        k.get("delta", delta.data_ptr()), k.get("ei", ei.ptr()), k.get("ldei", ei.ld),
                                        k.get("ws", ws.data_ptr()), k.get("n", ws.numel()), st)

    for bad in (dict(e=None), dict(e=ed.ptr() + 4), dict(lde=ed.ld + 2), dict(lde=n_out - 4), dict(ldx=n_out - 4), dict(ldx=xo.ld + 1),
                dict(x=None), dict(act=3), dict(act=-1), dict(d=None), dict(ldd=n_out - 4), dict(ldd=dd.ld + 2), dict(db_h=None),
                dict(rows=0), dict(ws=None), dict(d=ed.ptr(), ldd=ed.ld + 4)):
        assert site(**bad) == ERR_ARG, bad
    assert site(n=ws1.numel() - 16) == ERR_WS and b"workspace too small" in lib.kurbm_last_error()
    for bad in (dict(e=None), dict(e=ed.ptr() + 4), dict(lde=ed.ld + 2), dict(lde=n_out - 4), dict(xi=None), dict(ldin=n_in - 2),
                dict(ldin=xi.ld + 2), dict(xo=None), dict(ldout=n_out - 4), dict(act=3), dict(delta=None), dict(delta=delta.data_ptr() + 4),
                dict(ldei=n_in - 2), dict(ldei=ei.ld + 2), dict(ei=ei.ptr() + 4), dict(rows=0), dict(ws=None)):
        assert layer(**bad) == ERR_ARG, bad
    assert layer(n=ws.numel() - 16) == ERR_WS and b"workspace too small" in lib.kurbm_last_error()
    # the top layer's call
    Wt, bht, bvt = R.model(n_out, C, 20, std=.1)
    V, _ = R.labelled_batch(rows, n_out, C)
    top = _engine(gpu_device, Wt, bht, bvt)
    vd, et = _dm(V, gpu_device), _dm(np.full((rows, n_out), 7.0), gpu_device)
    tws, tdelta = top.disc_workspace(rows, C), top.delta_buffer()
    tdelta.fill_(7.0)
    TP = C_.byref(top.params)

    def disc(**k):
        return lib.kurbm_disc_backprop(ctx, TP, k.get("C", C), k.get("v", vd.ptr()), k.get("rows", rows), k.get("ldv", vd.ld),
                                       k.get("delta", tdelta.data_ptr()), k.get("ei", et.ptr()), k.get("ldei", et.ld), None,
                                       k.get("ws", tws.data_ptr()), k.get("n", tws.numel()), st)

    for bad in (dict(C=1), dict(C=65), dict(v=None), dict(ldv=vd.ld + 2), dict(ldv=vd.ld - 4), dict(delta=None), dict(ldei=n_out - 4),
                dict(ldei=et.ld + 2), dict(ei=et.ptr() + 4), dict(rows=0), dict(ws=None)):
        assert disc(**bad) == ERR_ARG, bad
    assert disc(n=tws.numel() - 16) == ERR_WS and b"workspace too small" in lib.kurbm_last_error()
    torch.cuda.synchronize()
    for t in (dd.view(), ei.view(), et.view(), db_h, delta, tdelta):
        assert bool((t == 7.0).all().item())
    assert _same(ed.to_numpy(), e) and _same(eng.get_weights()[0], W) and _same(top.get_weights()[0], Wt)
    # ... and the same calls with good arguments are accepted
    assert site() == 0 and layer() == 0 and disc() == 0
    torch.cuda.synchronize()
