"""Momentum and L2 weight decay fused into the launch that applies the CD update (include/kurbm.h: kurbm_momentum, the *_mom
entry points; csrc: the MOM instantiations of k_reduce_apply, k_reduce_apply_split, k_apply_delta).

    W   : vel <- mu vel + lr (g - lambda W) ;  W   <- W   + vel
    b_h : vel <- mu vel + lr g              ;  b_h <- b_h + vel        (no decay on biases; b_v likewise)

g is the packed sum the plain step emits, so the arithmetic is checked "teacher-forced": with the GPU's own g, elementwise in
float64, against bounds that count fp32 roundings -- and g itself is tied bit for bit to the delta of today's
cd_step(apply=False, emit_delta=True), the path the oracle already holds.

Shapes (the smallest that reach every branch):  S1 784 x 128, batch 128 -- the example's size, where 'auto' without momentum takes
the one-launch 'small' step;  S2 100 x 50, batch 36 -- n_hid % 4 != 0 (the two-launch fallback of the x3 / bf16 steps), tiles
hanging over both edges, bias-block tails (n_vis + n_hid no multiple of 32);  S3 200 x 136, batch 512 -- several tiles each way,
n_hid % 4 == 0 but no multiple of 64, more than one split-K slab."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"S1": (784, 128, 128), "S2": (100, 50, 36), "S3": (200, 136, 512)}
# the constants as the kernels see them (fp32), for the float64 arithmetic of the checks
MU, LAM, LR = 0.9, 1e-3, 0.01
MU32, LAM32, LR32 = (float(np.float32(x)) for x in (MU, LAM, LR))
SEED, STEP = 11, 3


def _problem(shape, grey=False, seed=5):
    nv, nh, B = SHAPES[shape]
    g = np.random.default_rng(seed)
    W = g.uniform(-0.1, 0.1, (nv, nh)).astype(np.float32)
    bh = g.uniform(-0.1, 0.1, nh).astype(np.float32)
    bv = g.uniform(-0.1, 0.1, nv).astype(np.float32)
    V = ((np.floor(g.random((B, nv)) * 256.0) / 255.0) if grey else (g.random((B, nv)) < 0.3)).astype(np.float32)
    vel = (g.uniform(-0.02, 0.02, (nv, nh)).astype(np.float32), g.uniform(-0.02, 0.02, nh).astype(np.float32),
           g.uniform(-0.02, 0.02, nv).astype(np.float32))
    return W, bh, bv, V, vel


def _engine(dev, W, bh, bv, vel=None):
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    e = DeviceRBM(W, bh, bv, dev)
    if vel is not None:
        e.set_velocity(*vel)
    return e


def _unpack(delta, nv, nh):
    d = delta.cpu().numpy()
    return d[:nv * nh].reshape(nv, nh), d[nv * nh:nv * nh + nh], d[nv * nh + nh:]


def _check_rule(name, p0, v0, g, p1, v1, lam):
    """vel' against mu vel + lr (g - lam p) and p' against p + vel', elementwise in float64, printing the worst ratio first.
    First bound: at most four fp32 roundings of 2^-24 each, doubled (holds with or without contraction to FMA); second: one
    rounding, doubled."""
    p0, v0, g, p1, v1 = (np.asarray(x, dtype=np.float64) for x in (p0, v0, g, p1, v1))
    want = MU32 * v0 + LR32 * (g - lam * p0)
    tol_v = 2.0 ** -21 * (np.abs(MU32 * v0) + np.abs(LR32 * g) + np.abs(LR32 * lam * p0))
    tol_p = 2.0 ** -23 * (np.abs(p0) + np.abs(v1))
    err_v, err_p = np.abs(v1 - want), np.abs(p1 - (p0 + v1))
    print("%s: worst |vel err| / bound %.3g, worst |param err| / bound %.3g"
          % (name, float(np.max(err_v / np.maximum(tol_v, 1e-300))), float(np.max(err_p / np.maximum(tol_p, 1e-300)))))
    assert np.all(err_v <= tol_v), name + ": velocity"
    assert np.all(err_p <= tol_p), name + ": parameter"


STEP_CASES = [(path, shape, False) for path in ("fp32", "x3", "bf16") for shape in ("S1", "S2", "S3")] + [("x3", "S2", True)]


@pytest.mark.parametrize("path,shape,gauss", STEP_CASES, ids=["%s-%s%s" % (p, s, "-gauss" if g else "") for p, s, g in STEP_CASES])
def test_one_step_teacher_forced(gpu_device, path, shape, gauss):
    from keras_unsupervised_amd.ebm.engine import MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, DeviceMatrix
    nv, nh, B = SHAPES[shape]
    W, bh, bv, V, vel = _problem(shape, grey=gauss)
    mode = MODE_VISIBLE_GAUSSIAN if gauss else MODE_VISIBLE_BERNOULLI
    Vd = DeviceMatrix.from_host(V, gpu_device)
    e = _engine(gpu_device, W, bh, bv, vel)
    e.cd_step(Vd, B, 0, LR, SEED, STEP, mode=mode, compute=path, emit_delta=True, momentum=(MU, LAM))
    torch.cuda.synchronize()
    gW, gbh, gbv = _unpack(e.delta, nv, nh)
    W1, bh1, bv1 = e.get_weights()
    vW1, vbh1, vbv1 = e.get_velocity()
    assert np.all(np.isfinite(W1)) and float(np.abs(gW).max()) > 0.0
    _check_rule("W", W, vel[0], gW, W1, vW1, LAM32)
    _check_rule("b_h", bh, vel[1], gbh, bh1, vbh1, 0.0)
    _check_rule("b_v", bv, vel[2], gbv, bv1, vbv1, 0.0)
    # g is, bit for bit, what today's emit-only step gives for the same counters
    twin = _engine(gpu_device, W, bh, bv)
    twin.cd_step(Vd, B, 0, LR, SEED, STEP, mode=mode, compute=path, apply=False, emit_delta=True)
    torch.cuda.synchronize()
    assert torch.equal(e.delta, twin.delta)
    assert twin.velocity is None
    # the padding columns [n_hid, ldw) of W stay zero
    assert e.W.ld >= nh and float(e.W.t[:, nh:].abs().sum()) == 0.0


@pytest.mark.parametrize("path,shape", [(p, s) for p in ("x3", "bf16") for s in ("S2", "S3")])
def test_mirror_follows_master(gpu_device, path, shape):
    """The bf16 pieces the momentum launch wrote (both orientations) are those of the new fp32 weights: a half step each way
    equals, bit for bit, the same call on a fresh engine built from get_weights()."""
    from keras_unsupervised_amd import _lib
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    nv, nh, B = SHAPES[shape]
    W, bh, bv, V, vel = _problem(shape)
    pieces = 3 if path == "x3" else 1
    Vd = DeviceMatrix.from_host(V, gpu_device)
    e = _engine(gpu_device, W, bh, bv, vel)
    e.cd_step(Vd, B, 0, LR, SEED, STEP, compute=path, momentum=(MU, LAM))
    assert e._mirrors[pieces][1] is False          # the engine trusts the mirror the launch wrote
    fresh = _engine(gpu_device, *e.get_weights())
    H = DeviceMatrix.from_host((np.random.default_rng(9).random((B, nh)) < 0.5).astype(np.float32), gpu_device)
    for direction, x in (("vh", Vd), ("hv", H)):
        a = e.half_step_bf16(direction, x, B, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, SEED, 0x100, 7, pieces=pieces, want_prob=True)
        b = fresh.half_step_bf16(direction, x, B, _lib.ACT_SIGMOID, _lib.NOISE_BERNOULLI, SEED, 0x100, 7, pieces=pieces, want_prob=True)
        torch.cuda.synchronize()
        assert torch.equal(a["prob"].t, b["prob"].t) and torch.equal(a["sample"].t, b["sample"].t), direction


@pytest.mark.parametrize("path", ["fp32", "x3", "bf16"])
def test_which_masks_parameters_and_velocities(gpu_device, path):
    from keras_unsupervised_amd import _lib
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    for shape in ("S2", "S3"):
        nv, nh, B = SHAPES[shape]
        W, bh, bv, V, vel = _problem(shape)
        e = _engine(gpu_device, W, bh, bv, vel)
        e.cd_step(DeviceMatrix.from_host(V, gpu_device), B, 0, LR, SEED, STEP, compute=path, which=_lib.WHICH_BH, momentum=(MU, LAM))
        W1, bh1, bv1 = e.get_weights()
        vW1, vbh1, vbv1 = e.get_velocity()
        assert np.array_equal(W1, W) and np.array_equal(bv1, bv) and np.array_equal(vW1, vel[0]) and np.array_equal(vbv1, vel[2])
        assert not np.array_equal(bh1, bh) and not np.array_equal(vbh1, vel[1])
        assert np.array_equal(bh1, (bh + vbh1).astype(np.float32))


@pytest.mark.parametrize("path", ["fp32", "x3", "bf16"])
def test_zero_momentum_zero_decay_is_the_plain_step(gpu_device, path):
    """mu = 0, lambda = 0 through the _mom entry point: vel' = fl(lr g) (one rounding, doubled: 2^-23 |lr g|), and W' = fl(W + vel')
    against the plain step's fl(W + lr g) (possibly one fused rounding): three roundings in all, each at most 2^-24 of a value no
    larger than |W| + |lr g|, doubled as in the one-step test -- inside 2^-21 |lr g| + 2^-22 (|W| + |vel'|)."""
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    for shape in ("S2", "S3"):
        nv, nh, B = SHAPES[shape]
        W, bh, bv, V, _ = _problem(shape)
        Vd = DeviceMatrix.from_host(V, gpu_device)
        e, plain = _engine(gpu_device, W, bh, bv), _engine(gpu_device, W, bh, bv)
        e.cd_step(Vd, B, 0, LR, SEED, STEP, compute=path, emit_delta=True, momentum=(0.0, 0.0))
        plain.cd_step(Vd, B, 0, LR, SEED, STEP, compute=path, emit_delta=True)
        torch.cuda.synchronize()
        assert torch.equal(e.delta, plain.delta)
        for p0, g, p1, q1, v1 in zip((W, bh, bv), _unpack(e.delta, nv, nh), e.get_weights(), plain.get_weights(), e.get_velocity()):
            p0, g, p1, q1, v1 = (np.asarray(x, dtype=np.float64) for x in (p0, g, p1, q1, v1))
            assert np.all(np.abs(v1 - LR32 * g) <= 2.0 ** -23 * np.abs(LR32 * g))
            assert np.all(np.abs(p1 - q1) <= 2.0 ** -21 * np.abs(LR32 * g) + 2.0 ** -22 * (np.abs(p0) + np.abs(v1)))


@pytest.mark.parametrize("path,shape", [("fp32", "S2"), ("x3", "S2"), ("x3", "S3")])
def test_epoch_call_equals_step_loop(gpu_device, path, shape):
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    nv, nh, B = SHAPES[shape]
    W, bh, bv, _, vel = _problem(shape)
    n = 2 * B + 20                                   # three batches, a ragged last one
    V = DeviceMatrix.from_host((np.random.default_rng(21).random((n, nv)) < 0.3).astype(np.float32), gpu_device)
    a, b = _engine(gpu_device, W, bh, bv, vel), _engine(gpu_device, W, bh, bv, vel)
    assert a.cd_epoch(V, n, B, LR, SEED, 40, compute=path, momentum=(MU, LAM)) == 3
    for i, lo in enumerate(range(0, n, B)):
        b.cd_step(V, min(B, n - lo), lo, LR, SEED, 40 + i, compute=path, momentum=(MU, LAM))
    for x, y in zip(a.get_weights() + a.get_velocity(), b.get_weights() + b.get_velocity()):
        assert np.array_equal(x, y)
    assert not np.array_equal(a.get_weights()[0], W)


class _Spy:
    """Stands in for DeviceRBM.lib and records the entry points that are looked up."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _fit_problem():
    nv, nh, B = SHAPES["S1"]
    W, bh, bv, _, _ = _problem("S1")
    V = (np.random.default_rng(31).random((2 * B + 40, nv)) < 0.3).astype(np.float32)
    return nv, nh, B, (W, bh, bv), V


def test_rbm_fit_with_a_momentum_schedule(gpu_device):
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    nv, nh, B, W0, V = _fit_problem()
    hps = {"batch_size": B, "epochs": 3, "lr": LR, "momentum": [0.5, 0.9], "weight_decay": LAM}
    r = RBM(hps, nh, mode=MODE_VISIBLE_BERNOULLI, seed=SEED, weights=W0, device=gpu_device, compute_dtype="auto")
    assert r.fit(V, verbose=0) is None
    path = r._compute()
    assert path != "small" and path in ("x3", "fp32")
    assert RBM(dict(hps, momentum=0.0, weight_decay=0.0), nh, mode=MODE_VISIBLE_BERNOULLI)._compute() == "small"
    # the same steps through DeviceRBM, mu = 0.5, 0.9, 0.9
    e = _engine(gpu_device, *W0)
    Vd = DeviceMatrix.from_host(V, gpu_device)
    windows = [(lo, min(B, len(V) - lo)) for lo in range(0, len(V), B)]
    planes = e.make_planes(Vd, windows) if path == "x3" else None
    step = 0
    for mu in (0.5, 0.9, 0.9):
        for lo, rows in windows:
            e.cd_step(Vd, rows, lo, LR, SEED, step, compute=path, planes=planes, momentum=(mu, LAM))
            step += 1
    for x, y in zip(r.get_weights() + list(r._dev.get_velocity()), list(e.get_weights()) + list(e.get_velocity())):
        assert np.array_equal(x, y)
    # a default RBM: no velocity, today's entry points and nothing else, today's bits
    d = RBM({"batch_size": B, "epochs": 3, "lr": LR}, nh, mode=MODE_VISIBLE_BERNOULLI, seed=SEED, weights=W0, device=gpu_device)
    d.build((None, nv))
    spy = d._dev.lib = _Spy(d._dev.lib)
    d.fit(V, verbose=0)
    assert d._dev.velocity is None and d._dev.get_velocity() is None
    assert "kurbm_cd_epoch_small" in spy.names and not [n for n in spy.names if n.endswith("_mom")]
    plain = _engine(gpu_device, *W0)
    for epoch in range(3):
        plain.cd_epoch(Vd, len(V), B, LR, SEED, 3 * epoch, compute="small")
    for x, y in zip(d.get_weights(), plain.get_weights()):
        assert np.array_equal(x, y)
    assert not np.array_equal(d.get_weights()[0], r.get_weights()[0])


def test_checkpoint_carries_the_velocity(gpu_device, tmp_path):
    from keras_unsupervised_amd.ebm import MODE_VISIBLE_BERNOULLI, RBM, load_rbm, save_rbm
    nv, nh, B, W0, V = _fit_problem()
    hps = {"batch_size": B, "epochs": 1, "lr": LR, "momentum": MU, "weight_decay": LAM}
    a = RBM(dict(hps), nh, mode=MODE_VISIBLE_BERNOULLI, seed=SEED, weights=W0, device=gpu_device)
    a.fit(V, verbose=0)
    save_rbm(a, str(tmp_path / "a"))
    b = load_rbm(str(tmp_path / "a"), device=gpu_device)
    assert b.momentum == MU and b.weight_decay == LAM
    for x, y in zip(a._dev.get_velocity(), b._dev.get_velocity()):
        assert np.array_equal(x, y)
    b.fit(V, verbose=0)
    straight = RBM(dict(hps, epochs=2), nh, mode=MODE_VISIBLE_BERNOULLI, seed=SEED, weights=W0, device=gpu_device)
    straight.fit(V, verbose=0)
    for x, y in zip(b.get_weights() + list(b._dev.get_velocity()), straight.get_weights() + list(straight._dev.get_velocity())):
        assert np.array_equal(x, y)
    # a checkpoint without velocity tensors (written before any momentum step): loads with a zero velocity, and fits
    c = RBM(dict(hps), nh, mode=MODE_VISIBLE_BERNOULLI, seed=SEED, weights=W0, device=gpu_device)
    c.build((None, nv))
    _, tensors = save_rbm(c, str(tmp_path / "c"))
    from safetensors.numpy import load_file
    assert not [k for k in load_file(tensors) if k.startswith("velocity")]
    c2 = load_rbm(str(tmp_path / "c"), device=gpu_device)
    assert c2._dev.get_velocity() is None
    c2.fit(V, verbose=0)
    for x, y in zip(c2.get_weights() + list(c2._dev.get_velocity()), a.get_weights() + list(a._dev.get_velocity())):
        assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def one_rank_comm(gpu_device):
    """A 1-rank RCCL communicator through the C ABI, as tests/test_gpu_parity.py builds it."""
    from keras_unsupervised_amd.ebm import dp
    comm = dp.Comm(gpu_device, 0, 1, dp.Comm.new_unique_id())
    yield comm
    comm.destroy()


def test_one_rank_exchange_equals_local_step(gpu_device, one_rank_comm):
    """emit -> all-reduce -> kurbm_x3_apply_delta_mom on one rank is the local kurbm_cd_step_x3_mom, bit for bit."""
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    nv, nh, B = SHAPES["S3"]
    W, bh, bv, V, vel = _problem("S3")
    Vd = DeviceMatrix.from_host(V, gpu_device)
    a, b = _engine(gpu_device, W, bh, bv, vel), _engine(gpu_device, W, bh, bv, vel)
    for step in (0, 1):
        a.cd_step_dp(one_rank_comm, Vd, B, 0, LR, SEED, step, compute="x3", momentum=(MU, LAM))
        b.cd_step(Vd, B, 0, LR, SEED, step, compute="x3", momentum=(MU, LAM))
    for x, y in zip(a.get_weights() + a.get_velocity(), b.get_weights() + b.get_velocity()):
        assert np.array_equal(x, y)
    assert not np.array_equal(a.get_weights()[0], W)


def test_refusals(gpu_device):
    """A null vel, mu = 1.0 and lambda < 0 each give KURBM_ERR_ARG from every momentum entry point, before anything is launched:
    the parameters are untouched."""
    from keras_unsupervised_amd import _lib
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix
    nv, nh, B = SHAPES["S3"]
    W, bh, bv, V, _ = _problem("S3")
    e = _engine(gpu_device, W, bh, bv)
    Vd = DeviceMatrix.from_host(V, gpu_device)
    vel = e.velocity_buffer()
    delta = e.delta_buffer()
    opts = _lib.CdOpts(1, 0, LR, 1, None, None, SEED, 0, STEP, 0)
    ws, mir = e.workspace(B), e.mirror(3)
    vp = e._x3_pieces(Vd, None, 0)
    wsb = e.workspace_bf16(B, 1, 3, vp)
    h, P, st = e.ctx.handle, C.byref(e.params), e._stream()
    bad = [_lib.Momentum(MU, LAM, None), _lib.Momentum(1.0, LAM, vel.data_ptr()), _lib.Momentum(MU, -1e-3, vel.data_ptr()),
           _lib.Momentum(MU, LAM, vel.data_ptr() + 4)]
    for m in bad:
        codes = [e.lib.kurbm_cd_step_mom(h, P, Vd.ptr(), B, Vd.ld, C.byref(opts), 7, ws.data_ptr(), ws.numel(), st, C.byref(m)),
                 e.lib.kurbm_cd_step_x3_mom(h, P, mir.data_ptr(), mir.numel(), Vd.ptr(), vp, B, Vd.ld, C.byref(opts), 7, wsb.data_ptr(),
                                            wsb.numel(), st, C.byref(m)),
                 e.lib.kurbm_cd_epoch_mom(h, P, Vd.ptr(), B, Vd.ld, B, C.byref(opts), ws.data_ptr(), ws.numel(), st, C.byref(m)),
                 e.lib.kurbm_apply_delta_mom(h, P, delta.data_ptr(), LR, 7, st, C.byref(m)),
                 e.lib.kurbm_x3_apply_delta_mom(h, P, mir.data_ptr(), mir.numel(), delta.data_ptr(), LR, 7, st, C.byref(m))]
        assert codes == [-1] * len(codes), (m.momentum, m.weight_decay, m.vel, codes)
        assert e.lib.kurbm_last_error()
    # a null block, and a step that does not apply
    assert e.lib.kurbm_cd_step_mom(h, P, Vd.ptr(), B, Vd.ld, C.byref(opts), 7, ws.data_ptr(), ws.numel(), st, None) == -1
    emit_only = _lib.CdOpts(1, 0, LR, 0, delta.data_ptr(), None, SEED, 0, STEP, 0)
    ok = _lib.Momentum(MU, LAM, vel.data_ptr())
    assert e.lib.kurbm_cd_step_mom(h, P, Vd.ptr(), B, Vd.ld, C.byref(emit_only), 7, ws.data_ptr(), ws.numel(), st, C.byref(ok)) == -1
    with pytest.raises(ValueError):
        e.cd_step(Vd, B, 0, LR, SEED, STEP, compute="small", momentum=(MU, LAM))
    torch.cuda.synchronize()
    for x, y in zip(e.get_weights(), (W, bh, bv)):
        assert np.array_equal(x, y)
    assert float(vel.abs().sum()) == 0.0
