"""Contract tests of the C ABI's buffer promises (include/kurbm.h, conventions block): guard bands, wide leading dimensions,
poisoned padding, refused sizes.

Every GPU case runs one call twice with the same counters -- (A) on an ordinary DeviceRBM, as the rest of the suite does, and
(B) on a GuardedRBM (tests/guarded.py): every buffer an arena carve of exactly the queried size between two guards of 0xFF,
every matrix with ld % 8 == 4 and ld >= cols + 4, input padding NaN, output padding a known finite word, scratch NaN -- and asserts
  1. arena.check(): no guard byte, no output padding word and no input byte (W's padding included) has changed;
  2. every result of B equals A bit for bit (no tolerance: layout and placement must not change a bit);
  3. B's result passes the oracle check the parity tests apply to that call (check_half_step, the float64 statistics check of
     test_cd_step_vs_oracle, ...), at their tolerances.
These are contract tests, not parity tests: the arithmetic is held by tests/test_gpu_parity.py; here it only anchors the pair.

Shapes (batch, n_vis, n_hid):  S0 1 x 5 x 3 (below one MFMA tile);  S1 36 x 100 x 50 (n_hid % 4 != 0: packed-velocity tail, the
two-launch momentum fallback, bias block tail);  S2 260 x 200 x 136 (four rows past a 256-row x3 tile, n_hid % 4 == 0 but not
% 64, several split-K slabs);  S3 50 x 70 x 90 and 128 x 784 x 128 (the two regimes of the one-launch small path).

entry point                                   shapes     buffers carved (B side)
--------------------------------------------  ---------  ----------------------------------------------------------------------
kurbm_half_step_{vh,hv}_dbg                   S0 S1 S2   W b_h b_v, input, sample / prob / u (wide ld_out); prob-only form
kurbm_half_step_x3 (0/1 and grey input)       S0 S1 S2   + x3 mirror, x3 workspace; S2 with KURBM_X3_TALL 0 and 1
kurbm_half_step_bf16                          S0 S1 S2   + bf16 mirror, bf16 workspace
kurbm_{bf16,x3}_mirror_refresh                S1 S2      mirror of exactly *_mirror_bytes from a W with NaN padding, a half step each way
kurbm_philox_uniform                          S0 S1 S2   wide patterned output
kurbm_bf16_exact                              S1         NaN-padded input, the flag word
kurbm_cd_step, _x3, _bf16 (+ their _mom)      S1 S2      W b_h b_v, batch, chain (in/out, wide), workspace, mirror, delta, velocity
kurbm_cd_epoch, _x3 (+ _mom)                  S1 S2      data of three batches (ragged last), workspace sized for the batch, chain
kurbm_x3_convert_rows                         S1 S2      planes of exactly n_windows * kurbm_x3_planes_bytes(max_rows), both v_pieces forms
kurbm_cd_step_small, kurbm_cd_epoch_small     S3         W b_h b_v, batch, workspace; KURBM_SMALL_LOCAL 1 and 0
kurbm_score_small                             S3         + score words, F of exactly 2 * rows floats; Bernoulli and Gaussian
kurbm_cd_epoch_small_scored                   S3         + scores: 2 * steps floats inside a patterned pinned host tensor
kurbm_free_energy, kurbm_free_energy_x3       S1 S2      v, F, workspace, mirror
kurbm_score_x3 (F given / F null)             S1 S2      v, score words, F of 2 * rows floats, workspace, mirror
kurbm_outer_delta                             S1 S2      four operands (wide), dense delta_w, workspace
kurbm_x3_dump_plane                           S1 S2      workspace of the step, wide output
kurbm_cd_step_x3_dp (n_chunks 0, 3), _bf16_dp S1 S2      as the steps, packed delta; 1-rank RCCL communicator
kurbm_apply_delta, kurbm_x3_apply_delta       S1 S2      packed delta (input), velocity (the _mom twins), mirror
undersized workspace / mirror / planes        S1         every entry point above that takes a size: refused, nothing changed
not covered                                              the hipIpc peer exchange (library-owned buffers, several processes)

The CPU-tier test at the top builds the arena on the CPU and shows that check() fails, naming buffer and side, when one byte is
flipped in a leading guard, a trailing guard, an output's padding and an input's padding.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import philox
from oracle import rbm_oracle as O
from oracle.make_golden import synthetic_binary, synthetic_params, synthetic_real

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # guarded.py and test_gpu_parity.py live beside this file
from guarded import OUT_WORD, Arena, GuardError, wide_ld

gpu = pytest.mark.gpu       # (per test, not `pytestmark`: the arena's self-test below belongs to the CPU tier)

TOL = 1e-4          # the bars of tests/test_gpu_parity.py
FLIP_BAND = 1e-5
SHAPES = {"S0": (1, 5, 3), "S1": (36, 100, 50), "S2": (260, 200, 136), "S3a": (50, 70, 90), "S3b": (128, 784, 128)}
MU, LAM, LR = 0.9, 1e-3, 0.01
SEED, STEP = 11, 3


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier: the harness can fail
# ---------------------------------------------------------------------------------------------------------------------
def test_arena_detects_every_kind_of_damage():
    a = Arena("cpu", capacity=24 << 20)
    raw = a.carve(1000, "raw")
    out = a.carve_matrix(5, 7, name="out")
    x = np.arange(15, dtype=np.float32).reshape(3, 5)
    inp = a.carve_matrix(3, 5, data=x, name="inp")
    last = a.carve(48, "last")
    assert raw.numel() == 1000 and raw.data_ptr() % 256 == 0 and last.numel() == 48
    for m, cols in ((out, 7), (inp, 5)):
        assert m.ld % 8 == 4 and m.ld >= cols + 4 and m.t.shape == (m.rows, m.ld) and m.t.data_ptr() % 256 == 0
    assert wide_ld(3) == 12 and wide_ld(50) == 60 and wide_ld(136) == 140 and wide_ld(100) == 108
    assert np.array_equal(inp.to_numpy(), x) and bool(torch.isnan(inp.t[:, 5:]).all())
    assert bool((out.t.view(torch.int32) == OUT_WORD - (1 << 32)).all()) and bool(torch.isfinite(out.t).all())
    first = a.bufs[0]
    assert first.off - a.base >= a.guard and a.buf.numel() - (a.bufs[-1].off + 48) >= a.guard >= 1 << 20
    a.check()
    out.t[:, :7] = 1.0            # an output's payload is the library's to write
    raw.fill_(3)
    a.check()
    flat = a.buf
    i_out, i_inp = a.bufs[1].off, a.bufs[2].off
    cases = [(first.off - 5, "raw: leading guard", "-5 .. -5"),
             (a.bufs[-1].off + 48 + 9, "last: trailing guard", "57 .. 57"),
             (i_out + (2 * out.ld + 8) * 4 + 1, "out: output padding", "row 2"),
             (i_inp + (1 * inp.ld + 6) * 4 + 2, "inp: input contents", "padding")]
    for pos, name, detail in cases:
        old = int(flat[pos].item())
        flat[pos] = old ^ 0x10
        with pytest.raises(GuardError) as ei:
            a.check()
        msg = str(ei.value)
        assert name in msg and detail in msg and msg.count("\n") == 1, msg
        flat[pos] = old
        a.check()
    # an in/out matrix (W, a persistent chain): payload free, padding pinned
    w = a.carve_matrix(4, 6, data=np.ones((4, 6), np.float32), name="W", kind="inout")
    w.t[:, :6] = 2.0
    a.check()
    w.t[3, 7] = 0.0
    with pytest.raises(GuardError, match="W: input padding"):
        a.check()
    w.t.view(torch.int32)[3, 7] = -1
    a.check()
    # a frozen raw buffer, and a payload byte of an input
    a.freeze(raw)
    raw[17] = 4
    with pytest.raises(GuardError, match=r"raw: input contents changed, 1 bytes, offsets 17 \.\. 17"):
        a.check()
    raw[17] = 3
    inp.t[0, 0] = 5.0
    with pytest.raises(GuardError, match="inp: input contents.*payload"):
        a.check()


# ---------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def one_rank_comm(gpu_device):
    """A 1-rank RCCL communicator through the C ABI, as tests/test_gpu_parity.py builds it."""
    from keras_unsupervised_amd.ebm import dp
    comm = dp.Comm(gpu_device, 0, 1, dp.Comm.new_unique_id())
    yield comm
    comm.destroy()


def rel_err(a, ref):
    return np.max(np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64))))


def check_half_step(out, p_ref, u_ref, s_ref):
    from test_gpu_parity import check_half_step as chk
    return chk(out, p_ref, u_ref, s_ref)


def eq(a, b, what):
    """Bit for bit."""
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: the guarded run differs from the plain run" % what


def grey3(rows, cols, seed):
    """Grey levels k / 255: not bf16 values, so the x3 path carries them as three pieces."""
    return (np.floor(synthetic_real(rows, cols, seed) * 256.0) / 255.0).astype(np.float32)


def grey_exact(rows, cols, seed):
    """Grey levels k / 256: bf16 values that are not all 0 / 1."""
    return (np.floor(synthetic_real(rows, cols, seed) * 256.0) / 256.0).astype(np.float32)


class Pair:
    """(A) a plain DeviceRBM and (B) a GuardedRBM in a fresh arena, from the same parameters."""

    def __init__(self, dev, W0, vel0=None):
        from guarded import GuardedRBM
        from keras_unsupervised_amd.ebm.engine import DeviceRBM
        self.dev, self.arena = dev, Arena(dev)
        self.A, self.B = DeviceRBM(*W0, dev), GuardedRBM(self.arena, *W0, dev)
        if vel0 is not None:
            self.A.set_velocity(*vel0)
            self.B.set_velocity(*vel0)

    def matrix(self, x, name, kind="input"):
        from keras_unsupervised_amd.ebm.engine import DeviceMatrix
        return DeviceMatrix.from_host(x, self.dev), self.arena.carve_matrix(x.shape[0], x.shape[1], data=x, name=name, kind=kind)

    def vector(self, x, name):
        """A dense fp32 input vector: (plain, carved and frozen)."""
        b = self.arena.carve_floats(x.size, name, data=x)
        self.arena.freeze(b)
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1)).to(self.dev), b

    def engines(self):
        return self.A, self.B

    def same_params(self):
        eq(self.A.W.view(), self.B.W.view(), "W")
        eq(self.A.b_h, self.B.b_h, "b_h")
        eq(self.A.b_v, self.B.b_v, "b_v")

    def same_extras(self):
        for name in ("delta", "velocity"):
            a, b = getattr(self.A, name), getattr(self.B, name)
            assert (a is None) == (b is None), name
            if a is not None:
                eq(a, b, name)

    def check(self):
        self.arena.check()
        self.A.check_status()


def _vel0(nv, nh, seed=5):
    g = np.random.default_rng(seed)
    return (g.uniform(-0.02, 0.02, (nv, nh)).astype(np.float32), g.uniform(-0.02, 0.02, nh).astype(np.float32),
            g.uniform(-0.02, 0.02, nv).astype(np.float32))


def _split(delta, nv, nh):
    return delta[: nv * nh].reshape(nv, nh), delta[nv * nh: nv * nh + nh], delta[nv * nh + nh:]


# ---------------------------------------------------------------------------------------------------------------------
# half steps
# ---------------------------------------------------------------------------------------------------------------------
HALF = ([("kurbm_half_step_vh_dbg+kurbm_half_step_hv_dbg", "fp32", s, None) for s in ("S0", "S1", "S2")]
        + [("kurbm_half_step_x3", d, s, None) for d in ("x3-binary", "x3-grey") for s in ("S0", "S1")]
        + [("kurbm_half_step_x3", d, "S2", t) for d in ("x3-binary", "x3-grey") for t in (0, 1)]
        + [("kurbm_half_step_bf16", "bf16", s, None) for s in ("S0", "S1", "S2")])


def _half(e, path, direction, x, rows, act, noise, sid, want_u=True, prob_only=False):
    if path == "fp32":
        return e.half_step(direction, x, rows, 0, act, noise, SEED, sid, STEP, row0=8, want_sample=not prob_only, want_prob=True,
                           want_u=want_u and not prob_only)
    return e.half_step_bf16(direction, x, rows, act, noise, SEED, sid, STEP, row0=8, pieces=3 if path.startswith("x3") else 1,
                            want_u=want_u)


@gpu
@pytest.mark.parametrize("entry,path,shape,tall", HALF,
                         ids=["%s-%s-%s%s" % (e, p, s, "" if t is None else "-tall%d" % t) for e, p, s, t in HALF])
def test_half_steps(gpu_device, ctx_option, entry, path, shape, tall):
    """Both directions at their sampling sites -- sigmoid + Bernoulli (v->h, h->v), relu + Bernoulli (v->h), linear + Gaussian
    (h->v) -- with sample, prob and u into wide patterned outputs, and the prob-only form; W, b_h, b_v must not change at all."""
    from keras_unsupervised_amd._lib import (ACT_LINEAR, ACT_RELU, ACT_SIGMOID, NOISE_BERNOULLI, NOISE_GAUSSIAN, NOISE_NONE)
    B, nv, nh = SHAPES[shape]
    if tall is not None:
        ctx_option("KURBM_X3_TALL", tall, -1)
    W, b_h, b_v = synthetic_params(nv, nh, seed=3100 + B)
    if path.startswith("x3"):
        W = (W * np.float32(3.7)).astype(np.float32)             # use all 24 significand bits
    v = {"fp32": synthetic_real, "bf16": synthetic_real, "x3-grey": grey3}.get(path, lambda r, c, s: synthetic_binary(r, c, s, p=0.3))(B, nv, 3101 + B)
    h = grey3(B, nh, 3102 + B) if path == "x3-grey" else synthetic_binary(B, nh, 3102 + B, p=0.5)
    # the oracle sees what the path multiplies: rounded operands on the bf16 path
    Wo, vo = (O.bf16_round(W), O.bf16_round(v)) if path == "bf16" else (W, v)
    p = Pair(gpu_device, (W, b_h, b_v))
    p.B.freeze_params()
    vA, vB = p.matrix(v, "v")
    hA, hB = p.matrix(h, "h")
    rng = O.Rng(SEED, STEP, row0=8)
    G = O.MODE_VISIBLE_GAUSSIAN
    sites = [("vh", ACT_SIGMOID, NOISE_BERNOULLI, 4, lambda: O.sample_hidden(vo, Wo, b_h, rng, 4)),
             ("hv", ACT_SIGMOID, NOISE_BERNOULLI, 5, lambda: O.sample_visible(h, Wo, b_v, rng, 5)),
             ("vh", ACT_RELU, NOISE_BERNOULLI, 6, lambda: O.sample_hidden(vo, Wo, b_h, rng, 6, G)),
             ("hv", ACT_LINEAR, NOISE_GAUSSIAN, 7, lambda: O.sample_visible(h, Wo, b_v, rng, 7, G))]
    for direction, act, noise, sid, ref in sites:
        xA, xB = (vA, vB) if direction == "vh" else (hA, hB)
        bern = noise == NOISE_BERNOULLI
        oa = _half(p.A, path, direction, xA, B, act, noise, sid, want_u=bern)
        ob = _half(p.B, path, direction, xB, B, act, noise, sid, want_u=bern)
        p.check()
        assert ob["sample"].ld == wide_ld(ob["sample"].cols) and p.B.W.ld == wide_ld(nh)
        for key in ("sample", "prob", "u"):
            assert (oa[key] is None) == (ob[key] is None)
            if oa[key] is not None:
                eq(oa[key].view(), ob[key].view(), "%s act %d noise %d: %s" % (direction, act, noise, key))
        if bern:
            check_half_step(ob, *ref())
        else:
            loc, _, s_ref = ref()
            assert np.max(np.abs(ob["prob"].to_numpy() - loc)) <= TOL
            assert np.max(np.abs(ob["sample"].to_numpy() - s_ref)) <= TOL
    for direction, xA, xB, ref in (("vh", vA, vB, lambda: O.hidden_prob(vo, Wo, b_h)), ("hv", hA, hB, lambda: O.visible_prob(h, Wo, b_v))):
        oa = _half(p.A, path, direction, xA, B, ACT_SIGMOID, NOISE_NONE, 0, prob_only=True)
        ob = _half(p.B, path, direction, xB, B, ACT_SIGMOID, NOISE_NONE, 0, prob_only=True)
        p.check()
        assert ob["sample"] is None and ob["u"] is None
        eq(oa["prob"].view(), ob["prob"].view(), direction + " prob only")
        assert np.max(np.abs(ob["prob"].to_numpy() - ref())) <= TOL


@gpu
@pytest.mark.parametrize("bytes_knob", [1, 0], ids=["bytes1", "bytes0"])
@pytest.mark.parametrize("shape", ["S0", "S1", "S2"])
def test_half_step_x3_byte_plane_input(gpu_device, ctx_option, shape, bytes_knob):
    """kurbm_half_step_x3 with in_pieces = 1 | KURBM_V_BINARY: the 0/1 input staged as the byte plane of the steps (one bf16 piece
    with KURBM_X3_BYTES=0), in a workspace of exactly kurbm_x3_workspace_bytes(..., 1 | KURBM_V_BINARY).  Both directions at the
    Bernoulli sites and the prob-only form: guards intact, guarded == plain, the parity bars of the other formats -- and, the
    products being the same exact numbers in the same order, bit for bit what the one-piece format gives."""
    from keras_unsupervised_amd._lib import ACT_SIGMOID, NOISE_BERNOULLI, NOISE_NONE
    B, nv, nh = SHAPES[shape]
    ctx_option("KURBM_X3_BYTES", bytes_knob, 1)
    W, b_h, b_v = synthetic_params(nv, nh, seed=3150 + B)
    W = (W * np.float32(3.7)).astype(np.float32)
    v, h = synthetic_binary(B, nv, 3151 + B, p=0.3), synthetic_binary(B, nh, 3152 + B, p=0.5)
    p = Pair(gpu_device, (W, b_h, b_v))
    p.B.freeze_params()
    vA, vB = p.matrix(v, "v")
    hA, hB = p.matrix(h, "h")
    rng = O.Rng(SEED, STEP, row0=8)

    def half(e, direction, x, noise, sid, fmt="bytes"):
        return e.half_step_bf16(direction, x, B, ACT_SIGMOID, noise, SEED, sid, STEP, row0=8, pieces=3, want_u=bool(noise), in_format=fmt)

    for direction, xA, xB, sid, ref in (("vh", vA, vB, 4, lambda: O.sample_hidden(v, W, b_h, rng, 4)),
                                        ("hv", hA, hB, 5, lambda: O.sample_visible(h, W, b_v, rng, 5))):
        oa, ob, o1 = half(p.A, direction, xA, NOISE_BERNOULLI, sid), half(p.B, direction, xB, NOISE_BERNOULLI, sid), \
            half(p.A, direction, xA, NOISE_BERNOULLI, sid, "bf16")
        p.check()
        for key in ("sample", "prob", "u"):
            eq(oa[key].view(), ob[key].view(), "%s bytes: %s" % (direction, key))
            eq(oa[key].view(), o1[key].view(), "%s bytes against one bf16 piece: %s" % (direction, key))
        check_half_step(ob, *ref())
    for direction, xA, xB, ref in (("vh", vA, vB, lambda: O.hidden_prob(v, W, b_h)), ("hv", hA, hB, lambda: O.visible_prob(h, W, b_v))):
        oa, ob = half(p.A, direction, xA, NOISE_NONE, 0), half(p.B, direction, xB, NOISE_NONE, 0)
        p.check()
        assert ob["sample"] is None and ob["u"] is None
        eq(oa["prob"].view(), ob["prob"].view(), direction + " bytes prob only")
        assert np.max(np.abs(ob["prob"].to_numpy() - ref())) <= TOL


MIRROR = [("kurbm_bf16_mirror_refresh", 1), ("kurbm_x3_mirror_refresh", 3)]


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("entry,pieces", MIRROR, ids=[m[0] for m in MIRROR])
def test_mirror_refresh_from_nan_padded_weights(gpu_device, entry, pieces, shape):
    """A mirror of exactly *_mirror_bytes (0xFF before the call) refreshed from a W whose padding is NaN, then a half step each
    way: a NaN that reached the k padding of either orientation shows in the probabilities."""
    from keras_unsupervised_amd import _lib
    B, nv, nh = SHAPES[shape]
    W, b_h, b_v = synthetic_params(nv, nh, seed=3200 + B)
    p = Pair(gpu_device, (W, b_h, b_v))
    p.B.freeze_params()
    fn_bytes = p.B.lib.kurbm_bf16_mirror_bytes if pieces == 1 else p.B.lib.kurbm_x3_mirror_bytes
    mir = p.B.mirror(pieces)                     # carve + kurbm_*_mirror_refresh
    assert mir.numel() == fn_bytes(p.B.ctx.handle, nv, nh) and p.arena._rec(mir).name == "mirror%d" % pieces
    p.check()
    # and once more through the C ABI, into the mirror that now holds the first result
    _lib.check(getattr(p.B.lib, entry)(p.B.ctx.handle, C.byref(p.B.params), mir.data_ptr(), mir.numel(), p.B._stream()))
    p.check()
    v, h = synthetic_real(B, nv, 3201 + B), synthetic_binary(B, nh, 3202 + B, p=0.5)
    Wq = O.bf16_round(W) if pieces == 1 else W
    for direction, x, ref in (("vh", v, O.hidden_prob(O.bf16_round(v) if pieces == 1 else v, Wq, b_h)), ("hv", h, O.visible_prob(h, Wq, b_v))):
        xA, xB = p.matrix(x, direction + "_in")
        oa = p.A.half_step_bf16(direction, xA, B, 0, 0, 0, 0, 0, pieces=pieces)
        ob = p.B.half_step_bf16(direction, xB, B, 0, 0, 0, 0, 0, pieces=pieces)
        p.check()
        eq(oa["prob"].view(), ob["prob"].view(), direction)
        assert np.max(np.abs(ob["prob"].to_numpy() - ref)) <= TOL


@gpu
@pytest.mark.parametrize("shape", ["S0", "S1", "S2"])
def test_kurbm_philox_uniform(gpu_device, shape):
    B, nv, nh = SHAPES[shape]
    p = Pair(gpu_device, synthetic_params(8, 8, 1))
    p.B.freeze_params()
    seed = (0xDEADBEEF << 32) | 0x12345678
    ua = p.A.philox_uniform(B, nh, seed, 0x80000005, 0xFFFFFFF0, row0=(1 << 33) + 4)
    ub = p.B.philox_uniform(B, nh, seed, 0x80000005, 0xFFFFFFF0, row0=(1 << 33) + 4)
    p.check()
    assert ub.ld == wide_ld(nh)
    eq(ua.view(), ub.view(), "uniforms")
    ref = philox.uniform(B, nh, seed, 0x80000005, 0xFFFFFFF0, row0=(1 << 33) + 4)
    assert np.array_equal(ub.to_numpy().view(np.uint32), ref.view(np.uint32))


@gpu
def test_kurbm_bf16_exact_ignores_nan_padding(gpu_device):
    """The flag of a NaN-padded matrix is the flag of the clean one: 0 for 0/1 data, 2 for bf16 values, 3 otherwise."""
    from keras_unsupervised_amd import _lib
    B, nv, _ = SHAPES["S1"]
    p = Pair(gpu_device, synthetic_params(8, 8, 1))
    p.B.freeze_params()
    for name, x, want in (("binary", synthetic_binary(B, nv, 3301, p=0.4), 0), ("bf16-exact", grey_exact(B, nv, 3302), 2),
                          ("real", synthetic_real(B, nv, 3303), 3)):
        xA, xB = p.matrix(x, name)
        flag = p.arena.carve_floats(1, "flag_" + name, zero=True, dtype=torch.int32)
        _lib.check(p.B.lib.kurbm_bf16_exact(p.B.ctx.handle, xB.ptr(), B, nv, xB.ld, flag.data_ptr(), p.B._stream()))
        p.check()
        clean = torch.zeros(1, dtype=torch.int32, device=gpu_device)
        _lib.check(p.A.lib.kurbm_bf16_exact(p.A.ctx.handle, xA.ptr(), B, nv, xA.ld, clean.data_ptr(), p.A._stream()))
        assert int(flag.item()) == int(clean.item()) == want, (name, int(flag.item()), int(clean.item()))


# ---------------------------------------------------------------------------------------------------------------------
# CD steps
# ---------------------------------------------------------------------------------------------------------------------
CD_PATHS = {"fp32": "kurbm_cd_step", "x3-binary": "kurbm_cd_step_x3", "x3-grey": "kurbm_cd_step_x3", "x3-gauss": "kurbm_cd_step_x3",
            "bf16": "kurbm_cd_step_bf16"}
CD_VARIANTS = ["k1-apply", "k3-chain", "emit", "which2", "mom", "mom-which2"]


def _cd_problem(path, shape, n_rows=None, seed=3400):
    B, nv, nh = SHAPES[shape]
    n = n_rows or B
    W0 = synthetic_params(nv, nh, seed=seed + B)
    if path == "x3-grey":
        V, mode = grey3(n, nv, seed + 1 + B), O.MODE_VISIBLE_BERNOULLI
    elif path == "x3-gauss":
        V, mode = synthetic_real(n, nv, seed + 1 + B), O.MODE_VISIBLE_GAUSSIAN
    else:
        V, mode = synthetic_binary(n, nv, seed + 1 + B, p=0.3), O.MODE_VISIBLE_BERNOULLI
    return W0, V, mode, ("x3" if path.startswith("x3") else path)


def _mirror_follows(p, compute, V, vA, vB, rows):
    """The mirror the step left is that of the new weights: a prob-only half step, A against B and against the oracle."""
    if compute not in ("x3", "bf16"):
        return
    pieces = 3 if compute == "x3" else 1
    oa = p.A.half_step_bf16("vh", vA, rows, 0, 0, 0, 0, 0, pieces=pieces)
    ob = p.B.half_step_bf16("vh", vB, rows, 0, 0, 0, 0, 0, pieces=pieces)
    p.check()
    eq(oa["prob"].view(), ob["prob"].view(), "half step on the mirror the step left")
    Wn, bhn, _ = p.B.get_weights()
    ref = O.hidden_prob(O.bf16_round(V[:rows]), O.bf16_round(Wn), bhn) if pieces == 1 else O.hidden_prob(V[:rows], Wn, bhn)
    assert np.max(np.abs(ob["prob"].to_numpy() - ref)) <= TOL


@gpu
@pytest.mark.parametrize("variant", CD_VARIANTS)
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("path", list(CD_PATHS), ids=["%s-%s" % (v, k) for k, v in CD_PATHS.items()])
def test_cd_step(gpu_device, path, shape, variant):
    B, nv, nh = SHAPES[shape]
    W0, V, mode, compute = _cd_problem(path, shape)
    mom = variant.startswith("mom")
    vel0 = _vel0(nv, nh) if mom else None
    p = Pair(gpu_device, W0, vel0)
    vA, vB = p.matrix(V, "v_batch")
    chain0 = cA = cB = None
    kw = dict(mode=mode, compute=compute)
    if variant == "k3-chain":
        chain0 = synthetic_real(B, nv, 3402 + B) if mode == O.MODE_VISIBLE_GAUSSIAN else synthetic_binary(B, nv, 3402 + B, p=0.5)
        cA, cB = p.matrix(chain0, "v_chain", kind="inout")
        assert cB.ld == vB.ld
        kw.update(k=3)
    if variant == "emit":
        kw.update(apply=False, emit_delta=True)
    if variant.endswith("which2"):
        kw.update(which=2)
        p.B.freeze_params(b_h=False)           # W, b_v and their padding must not change at all
    if mom:
        kw.update(momentum=(MU, LAM), emit_delta=(variant == "mom"))      # (the same launch emits g)
    p.A.cd_step(vA, B, 0, LR, SEED, STEP, v_chain=cA, **kw)
    p.B.cd_step(vB, B, 0, LR, SEED, STEP, v_chain=cB, **kw)
    p.check()
    p.same_params()
    p.same_extras()
    if cA is not None:
        eq(cA.view(), cB.view(), "v_chain")
    Wn, bhn, bvn = p.B.get_weights()
    if variant == "emit":
        for x, x0 in zip((Wn, bhn, bvn), W0):
            assert np.array_equal(x, x0)
        dW, dbh, dbv = _split(p.B.delta.cpu().numpy(), nv, nh)
        if compute == "bf16":
            _, _, _, ch, (dW_ref, dbh_ref, dbv_ref) = O.cd_step_fused_bf16(*W0, V, LR, SEED, STEP)
            assert rel_err(dW, dW_ref) <= 2e-3 and rel_err(dbh, dbh_ref) <= TOL and np.array_equal(dbv, dbv_ref)
        else:
            _, _, _, ch, ref = O.cd_step_fused(*W0, V, LR, SEED, STEP, mode=mode)
            if path in ("x3-grey", "x3-gauss"):     # real-valued sums: the reference in float64, as test_cd_step_vs_oracle has it
                ref = O.cd_statistics({k_: ch[k_].astype(np.float64) for k_ in ("v_pos", "h_pos", "v_neg", "h_neg")})
            for got, want in zip((dW, dbh, dbv), ref):
                assert rel_err(got, want) <= TOL
    elif variant.endswith("which2"):
        assert np.array_equal(Wn, W0[0]) and np.array_equal(bvn, W0[2]) and not np.array_equal(bhn, W0[1])
        if mom:         # the velocity of a variable `which` leaves out is neither read nor written
            vW, vbh, vbv = p.B.get_velocity()
            assert np.array_equal(vW, vel0[0]) and np.array_equal(vbv, vel0[2]) and not np.array_equal(vbh, vel0[1])
    else:
        assert np.isfinite(Wn).all() and not np.array_equal(Wn, W0[0])
        _mirror_follows(p, compute, V, vA, vB, B)


# ---------------------------------------------------------------------------------------------------------------------
# epoch calls and resident planes
# ---------------------------------------------------------------------------------------------------------------------
EPOCH = [("kurbm_cd_epoch", "fp32", False, False, True), ("kurbm_cd_epoch_mom", "fp32", False, True, False),
         ("kurbm_cd_epoch_x3", "x3-binary", False, False, True), ("kurbm_cd_epoch_x3", "x3-gauss", False, False, False),
         ("kurbm_x3_convert_rows+kurbm_cd_epoch_x3", "x3-binary", True, False, False),
         ("kurbm_x3_convert_rows+kurbm_cd_epoch_x3", "x3-grey", True, False, False),
         ("kurbm_cd_epoch_x3_mom", "x3-binary", False, True, False),
         ("kurbm_x3_convert_rows+kurbm_cd_epoch_x3_mom", "x3-grey", True, True, False)]


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("entry,path,resident,mom,pcd", EPOCH,
                         ids=["%s-%s%s" % (e, p, "-chain" if c else "") for e, p, _, _, c in EPOCH])
def test_cd_epoch(gpu_device, entry, path, resident, mom, pcd, shape):
    """Two full batches and a remainder of 20 rows in one call, the workspace sized for the batch; with resident planes of
    exactly n_windows * kurbm_x3_planes_bytes(batch) bytes (the remainder window has its own, smaller layout)."""
    B, nv, nh = SHAPES[shape]
    N = 2 * B + 20
    W0, V, mode, compute = _cd_problem(path, shape, n_rows=N, seed=3500)
    p = Pair(gpu_device, W0, _vel0(nv, nh) if mom else None)
    vA, vB = p.matrix(V, "V")
    cA = cB = None
    k = 1
    if pcd:
        cA, cB = p.matrix(synthetic_binary(B, nv, 3502 + B, p=0.5), "v_chain", kind="inout")
        k = 2
    windows = [(lo, hi - lo) for lo, hi in O.batch_slices(N, B)]
    assert windows[-1] == (2 * B, 20) and len(windows) == 3
    got = []
    for e, v, c in ((p.A, vA, cA), (p.B, vB, cB)):
        planes = None
        if resident:
            planes = e.make_planes(v, windows, mode)
            assert planes is not None and planes.uniform(0, N, B) and planes.v_pieces == (3 if path == "x3-grey" else 1 | 0x10)
            assert planes.buf.numel() == 3 * int(e.lib.kurbm_x3_planes_bytes(e.ctx.handle, B, nv, planes.v_pieces))
            if e is p.B:
                p.arena.freeze(planes.buf)      # the steps only read them
                p.check()
        got.append(e.cd_epoch(v, N, B, LR, SEED, STEP, k=k, mode=mode, v_chain=c, compute=compute, planes=planes,
                              momentum=(MU, LAM) if mom else None))
    assert got == [3, 3]
    p.check()
    p.same_params()
    p.same_extras()
    if cA is not None:
        eq(cA.view(), cB.view(), "v_chain")
    Wn = p.B.get_weights()[0]
    assert np.isfinite(Wn).all() and not np.array_equal(Wn, W0[0])
    _mirror_follows(p, compute, V, vA, vB, B)


# ---------------------------------------------------------------------------------------------------------------------
# the one-launch small path
# ---------------------------------------------------------------------------------------------------------------------
SMALL = ["kurbm_cd_step_small", "kurbm_cd_epoch_small", "kurbm_score_small-bernoulli", "kurbm_score_small-gaussian",
         "kurbm_cd_epoch_small_scored"]


@gpu
@pytest.mark.parametrize("local", [1, 0])
@pytest.mark.parametrize("shape", ["S3a", "S3b"])
@pytest.mark.parametrize("entry", SMALL)
def test_small_path(gpu_device, ctx_option, entry, shape, local):
    from keras_unsupervised_amd._lib import CdOpts
    from keras_unsupervised_amd.ebm.engine import CHAIN_SCORE
    ctx_option("KURBM_SMALL_LOCAL", local, 1)
    B, nv, nh = SHAPES[shape]
    N = 2 * B + 20
    gauss = entry.endswith("gaussian")
    mode = O.MODE_VISIBLE_GAUSSIAN if gauss else O.MODE_VISIBLE_BERNOULLI
    W0 = synthetic_params(nv, nh, seed=3600 + B)
    V = synthetic_binary(N, nv, 3601 + B, p=0.3)
    p = Pair(gpu_device, W0)
    vA, vB = p.matrix(V, "V")
    if entry == "kurbm_cd_step_small":
        for e, v in ((p.A, vA), (p.B, vB)):
            e.cd_step(v, B, 0, 1e-3, 9, 0, mode=mode, compute="small")
        ref = O.cd_step_fused(*W0, V[:B], 1e-3, 9, 0, mode=mode)[:3]
        for a, b in zip(p.B.get_weights(), ref):
            assert np.max(np.abs(a - b)) <= TOL
    elif entry == "kurbm_cd_epoch_small":
        for e, v in ((p.A, vA), (p.B, vB)):
            assert e.cd_epoch(v, N, B, 1e-3, 9, 0, mode=mode, compute="small") == 3
    elif entry.startswith("kurbm_score_small"):
        p.B.freeze_params()
        sa, Fa = p.A.score_small(vA, B, 0, 7, 3, mode, CHAIN_SCORE, want_F=True)
        sb, Fb = p.B.score_small(vB, B, 0, 7, 3, mode, CHAIN_SCORE, want_F=True)
        p.check()
        assert Fb.numel() == 2 * B and p.arena._rec(Fb).nbytes == 8 * B
        eq(sa[:1], sb[:1], "score")
        eq(Fa, Fb, "F")
        got, want = float(sb[0].item()), O.step_score(*W0, V[:B], 7, 3, mode)
        assert abs(got - want) <= 1e-3 * max(1.0, abs(want)), (got, want)
        assert rel_err(Fb.cpu().numpy()[0], O.free_energy(V[:B], *W0)) <= TOL
    else:   # kurbm_cd_epoch_small_scored: B's scores are exactly 2 * steps floats inside a patterned pinned host tensor
        na, sa = p.A.cd_epoch_small_scored(vA, N, B, 1e-3, 9, 0, mode, CHAIN_SCORE)
        pad, steps = 64, 3
        host = torch.empty(2 * steps + 2 * pad, dtype=torch.float32, pin_memory=True)
        host.view(torch.int32).fill_(OUT_WORD - (1 << 32))
        e = p.B
        with torch.cuda.device(gpu_device):
            ws = e.workspace(B)
            opts = CdOpts(1, int(mode), 1e-3, 1, None, None, 9, 0, 0, 0)
            nb = e.lib.kurbm_cd_epoch_small_scored(e.ctx.handle, C.byref(e.params), vB.ptr(), N, vB.ld, B, C.byref(opts),
                                                   int(CHAIN_SCORE), host.data_ptr() + 4 * pad, ws.data_ptr(), ws.numel(), e._stream())
        torch.cuda.synchronize()
        assert na == nb == steps, (na, nb, e.lib.kurbm_last_error())
        hb = host.view(torch.int32)
        assert bool((hb[:pad] == OUT_WORD - (1 << 32)).all()) and bool((hb[pad + 2 * steps:] == OUT_WORD - (1 << 32)).all()), \
            "the scores' neighbours in the pinned tensor changed"
        eq(sa.reshape(-1), host[pad:pad + 2 * steps], "scores")
        assert bool((sa[:, 1] == 1.0).all()) and bool(torch.isfinite(sa).all())
    p.check()
    p.B.check_status()
    p.same_params()


# ---------------------------------------------------------------------------------------------------------------------
# free energy, score, statistics GEMM, plane dump
# ---------------------------------------------------------------------------------------------------------------------
FE = [("kurbm_free_energy", "real", None), ("kurbm_free_energy_x3", "binary", "x3"), ("kurbm_free_energy_x3", "grey", "x3")]


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("entry,data,compute", FE, ids=["%s-%s" % (e, d) for e, d, _ in FE])
def test_free_energy(gpu_device, entry, data, compute, shape):
    B, nv, nh = SHAPES[shape]
    W0 = synthetic_params(nv, nh, seed=3700 + B)
    V = {"real": synthetic_real, "grey": grey3}.get(data, lambda r, c, s: synthetic_binary(r, c, s, p=0.3))(B, nv, 3701 + B)
    p = Pair(gpu_device, W0)
    p.B.freeze_params()
    vA, vB = p.matrix(V, "v")
    Fa, Fb = p.A.free_energy(vA, B, compute=compute), p.B.free_energy(vB, B, compute=compute)
    p.check()
    assert p.arena._rec(Fb).nbytes == 4 * B
    eq(Fa, Fb, "F")
    ref = O.free_energy(*(x.astype(np.float64) for x in (V, W0[0], W0[1], W0[2])))
    assert rel_err(Fb.cpu().numpy(), ref) <= TOL


def _score_x3(e, v, rows, mode, chain, out, F):
    from keras_unsupervised_amd._lib import CdOpts, check
    with torch.cuda.device(e.device):
        vp = e._x3_pieces(v, None, mode)
        mir, ws = e.mirror(3), e.workspace_bf16(rows, 1, 3, vp)
        opts = CdOpts(1, int(mode), 0.0, 0, None, None, 7, 0, 3, int(chain))
        check(e.lib.kurbm_score_x3(e.ctx.handle, C.byref(e.params), mir.data_ptr(), mir.numel(), v.ptr(), vp, rows, v.ld, C.byref(opts),
                                   out.data_ptr(), F.data_ptr(), ws.data_ptr(), ws.numel(), e._stream()))


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("data", ["binary", "gaussian"])
@pytest.mark.parametrize("entry", ["kurbm_score_x3-F", "kurbm_score_x3-noF"])
def test_score_x3(gpu_device, entry, data, shape):
    from keras_unsupervised_amd.ebm.engine import CHAIN_SCORE
    B, nv, nh = SHAPES[shape]
    mode = O.MODE_VISIBLE_GAUSSIAN if data == "gaussian" else O.MODE_VISIBLE_BERNOULLI
    W0 = synthetic_params(nv, nh, seed=3800 + B)
    V = synthetic_real(B, nv, 3801 + B) if data == "gaussian" else synthetic_binary(B, nv, 3801 + B, p=0.3)
    p = Pair(gpu_device, W0)
    p.B.freeze_params()
    vA, vB = p.matrix(V, "v")
    if entry.endswith("noF"):
        sa, sb = p.A.score_x3(vA, B, 0, 7, 3, mode, CHAIN_SCORE), p.B.score_x3(vB, B, 0, 7, 3, mode, CHAIN_SCORE)
    else:
        sa = torch.empty(4, dtype=torch.float32, device=gpu_device)
        Fa = torch.empty(2 * B, dtype=torch.float32, device=gpu_device)
        sb, Fb = p.arena.carve_floats(4, "score"), p.arena.carve_floats(2 * B, "F")
        _score_x3(p.A, vA, B, mode, CHAIN_SCORE, sa, Fa)
        _score_x3(p.B, vB, B, mode, CHAIN_SCORE, sb, Fb)
    p.check()
    eq(sa[:1], sb[:1], "score")
    got, want = float(sb[0].item()), O.step_score(*W0, V, 7, 3, mode)
    assert abs(got - want) <= 1e-3 * max(1.0, abs(want)), (got, want)
    if entry.endswith("-F"):
        eq(Fa, Fb, "F")
        assert rel_err(Fb.cpu().numpy()[:B], O.free_energy(V, *W0)) <= TOL


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_kurbm_outer_delta(gpu_device, shape):
    B, nv, nh = SHAPES[shape]
    p = Pair(gpu_device, synthetic_params(nv, nh, seed=3900 + B))
    p.B.freeze_params()
    ops = [synthetic_binary(B, nv, 3901 + B, p=0.3), synthetic_binary(B, nh, 3902 + B, p=0.5), synthetic_binary(B, nv, 3903 + B, p=0.4),
           synthetic_real(B, nh, 3904 + B)]
    mats = [p.matrix(x, name) for x, name in zip(ops, ("v_pos", "h_pos", "v_neg", "h_neg"))]
    da = p.A.outer_delta(*[m[0] for m in mats], B)
    db = p.B.outer_delta(*[m[1] for m in mats], B)
    p.check()
    assert p.arena._rec(db).nbytes == 4 * nv * nh
    eq(da, db, "delta_w")
    o64 = [x.astype(np.float64) for x in ops]
    assert rel_err(db.cpu().numpy(), o64[0].T @ o64[1] - o64[2].T @ o64[3]) <= TOL


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("path", ["x3-binary", "x3-gauss"])
def test_kurbm_x3_dump_plane(gpu_device, path, shape):
    """The five planes a complete x3 CD-1 step left in a workspace of exactly the queried size, decoded into wide outputs."""
    from keras_unsupervised_amd import _lib
    B, nv, nh = SHAPES[shape]
    W0, V, mode, compute = _cd_problem(path, shape, seed=4000)
    p = Pair(gpu_device, W0)
    vA, vB = p.matrix(V, "v_batch")
    for e, v in ((p.A, vA), (p.B, vB)):
        e.cd_step(v, B, 0, LR, SEED, STEP, mode=mode, compute="x3", apply=False, emit_delta=True)
    p.check()
    p.B.freeze_params()
    planes = {}
    for which in (_lib.PLANE_H_POS, _lib.PLANE_H_POS_T, _lib.PLANE_V_NEG, _lib.PLANE_V_NEG_T, _lib.PLANE_H_NEG_T):
        a, b = p.A.dump_plane(which, vA, B, mode), p.B.dump_plane(which, vB, B, mode)
        p.check()
        assert b.ld == wide_ld(b.cols)
        eq(a.view(), b.view(), "plane %d" % which)
        planes[which] = b.to_numpy()
        assert np.isfinite(planes[which]).all()
    assert np.array_equal(planes[_lib.PLANE_H_POS], planes[_lib.PLANE_H_POS_T])
    # the states are the oracle's (teacher-forced on the GPU's own h_pos, as the parity tests do)
    p_ref, u_ref, h_ref = O.sample_hidden(V, *W0[:2], O.Rng(SEED, STEP), O.stream_h(0), mode)
    diff = planes[_lib.PLANE_H_POS] != h_ref
    assert np.all(np.abs(u_ref[diff] - p_ref[diff]) < FLIP_BAND), "h_pos differs from the oracle outside the rounding band"


# ---------------------------------------------------------------------------------------------------------------------
# the one-rank exchange forms
# ---------------------------------------------------------------------------------------------------------------------
DP = [("kurbm_cd_step_x3_dp", "x3", 0), ("kurbm_cd_step_x3_dp", "x3", 3), ("kurbm_cd_step_bf16_dp", "bf16", 0)]


@gpu
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("entry,compute,n_chunks", DP, ids=["%s-chunks%d" % (e, n) for e, _, n in DP])
def test_dp_step_one_rank(gpu_device, one_rank_comm, entry, compute, n_chunks, shape):
    B, nv, nh = SHAPES[shape]
    W0, V, mode, _ = _cd_problem("x3-binary", shape, seed=4100)
    p = Pair(gpu_device, W0)
    vA, vB = p.matrix(V, "v_batch")
    chain0 = synthetic_binary(B, nv, 4102 + B, p=0.5)
    cA, cB = p.matrix(chain0, "v_chain", kind="inout")
    for e, v, c in ((p.A, vA, cA), (p.B, vB, cB)):
        e.cd_step_dp(one_rank_comm, v, B, 0, LR, SEED, STEP, k=2, mode=mode, row0=8, v_chain=c, compute=compute, n_chunks=n_chunks)
    p.check()
    p.same_params()
    p.same_extras()
    eq(cA.view(), cB.view(), "v_chain")
    assert p.arena._rec(p.B.delta).nbytes == 4 * (nv * nh + nh + nv)
    # the summed statistics (one rank: this rank's) and the chain against the oracle, as the parity tests of each path hold them
    dW, dbh, dbv = _split(p.B.delta.cpu().numpy(), nv, nh)
    if compute == "bf16":
        _, _, _, ch, (dW_ref, dbh_ref, dbv_ref) = O.cd_step_fused_bf16(*W0, V, LR, SEED, STEP, k=2, row0=8, v_chain=chain0)
        assert rel_err(dW, dW_ref) <= 2e-3 and rel_err(dbh, dbh_ref) <= TOL and np.array_equal(dbv, dbv_ref)
    else:
        _, _, _, ch, ref = O.cd_step_fused(*W0, V, LR, SEED, STEP, k=2, row0=8, v_chain=chain0)
        for got, want in zip((dW, dbh, dbv), ref):
            assert rel_err(got, want) <= TOL
    assert np.array_equal(cB.to_numpy(), ch["v_neg"])
    _mirror_follows(p, compute, V, vA, vB, B)


APPLY = [("kurbm_apply_delta", None, False), ("kurbm_apply_delta_mom", None, True), ("kurbm_x3_apply_delta", "x3", False),
         ("kurbm_x3_apply_delta_mom", "x3", True)]


@gpu
@pytest.mark.parametrize("which", [7, 2])
@pytest.mark.parametrize("shape", ["S1", "S2"])
@pytest.mark.parametrize("entry,compute,mom", APPLY, ids=[a[0] for a in APPLY])
def test_apply_delta(gpu_device, entry, compute, mom, shape, which):
    """The apply after an exchange, on a carved packed delta (an input: it must not change).  Arithmetic: the rule in float64,
    elementwise; momentum at the bounds of tests/test_momentum_gpu.py (four roundings of 2^-24, doubled; one, doubled), the plain
    x + lr g at two roundings of 2^-24 (the product, the sum), doubled."""
    B, nv, nh = SHAPES[shape]
    W0 = synthetic_params(nv, nh, seed=4200 + B)
    vel0 = _vel0(nv, nh) if mom else None
    g = np.random.default_rng(4201 + B).uniform(-3.0, 3.0, nv * nh + nh + nv).astype(np.float32)
    p = Pair(gpu_device, W0, vel0)
    dA, dB = p.vector(g, "packed_delta")
    if compute == "x3":
        p.A.mirror(3), p.B.mirror(3)
    if which == 2:
        p.B.freeze_params(b_h=False)
    kw = dict(which=which, compute=compute, momentum=(MU, LAM) if mom else None)
    p.A.apply_delta(LR, delta=dA, **kw)
    p.B.apply_delta(LR, delta=dB, **kw)
    p.check()
    p.same_params()
    p.same_extras()
    new = p.B.get_weights()
    vel1 = p.B.get_velocity() if mom else (None, None, None)
    lr32, mu32, lam32 = (float(np.float32(x)) for x in (LR, MU, LAM))
    for i, (name, x0, gi, lam) in enumerate(zip(("W", "b_h", "b_v"), W0, _split(g, nv, nh), (lam32, 0.0, 0.0))):
        if not which & (1 << i):
            assert np.array_equal(new[i], x0), name
            if mom:
                assert np.array_equal(vel1[i], vel0[i]), name + " velocity"
            continue
        x0_, gi_ = x0.astype(np.float64), gi.astype(np.float64)
        if mom:
            v0_, v1_ = vel0[i].astype(np.float64), vel1[i].astype(np.float64)
            want = mu32 * v0_ + lr32 * (gi_ - lam * x0_)
            assert np.all(np.abs(v1_ - want) <= 2.0 ** -21 * (np.abs(mu32 * v0_) + np.abs(lr32 * gi_) + np.abs(lr32 * lam * x0_))), name
            assert np.all(np.abs(new[i] - (x0_ + v1_)) <= 2.0 ** -23 * (np.abs(x0_) + np.abs(v1_))), name
        else:
            assert np.all(np.abs(new[i] - (x0_ + lr32 * gi_)) <= 2.0 ** -22 * (np.abs(x0_) + np.abs(lr32 * gi_))), name
    if compute == "x3":
        V = synthetic_binary(B, nv, 4203 + B, p=0.3)
        vA, vB = p.matrix(V, "v")
        _mirror_follows(p, "x3", V, vA, vB, B)


# ---------------------------------------------------------------------------------------------------------------------
# undersized buffers are refused before anything is enqueued
# ---------------------------------------------------------------------------------------------------------------------
class Rig:
    """One guarded S1 engine with every buffer of every path carved and frozen; call(entry, short) passes the size named
    `short` 16 bytes below its query."""

    def __init__(self, dev, comm):
        from keras_unsupervised_amd import _lib
        from keras_unsupervised_amd._lib import CdOpts, Momentum, Rng
        B, nv, nh = SHAPES["S1"]
        self.B, self.nv, self.nh, self.N = B, nv, nh, 2 * B + 20
        p = self.p = Pair(dev, synthetic_params(nv, nh, seed=4300), _vel0(nv, nh))
        e = self.e = p.B
        self.comm = comm
        self.V = p.matrix(synthetic_binary(self.N, nv, 4301, p=0.3), "V")[1]
        self.H = p.matrix(synthetic_binary(B, nh, 4302, p=0.5), "H")[1]
        self.vp = e._x3_pieces(self.V, None, 0)
        assert self.vp == 1 | _lib.V_BINARY
        with torch.cuda.device(dev):
            # "ws": exactly the query; "wsw": what a step on this (wide) batch needs on top of it (include/kurbm.h, kurbm_workspace_bytes)
            self.buf = {"ws": p.arena.carve(e.lib.kurbm_workspace_bytes(e.ctx.handle, B, nv, nh, 1), "workspace_query"),
                        "wsw": e.workspace(B, 1, self.V.ld), "wsb": e.workspace_bf16(B, 1, 1, 1), "wsx": e.workspace_bf16(B, 1, 3, self.vp),
                        "mir1": e.mirror(1), "mir3": e.mirror(3)}
            self.buf["planes"] = p.arena.carve(e.lib.kurbm_x3_planes_bytes(e.ctx.handle, B, nv, self.vp), "planes")
        self.delta, self.vel = e.delta_buffer(), e.velocity_buffer()
        self.F, self.score = p.arena.carve_floats(2 * B, "F"), p.arena.carve_floats(4, "score")
        self.out = p.arena.carve_matrix(B, max(nv, nh), name="out")
        self.dense = p.arena.carve_floats(nv * nh, "delta_w")
        self.host = torch.zeros(64, dtype=torch.float32, pin_memory=True)
        self.opts = CdOpts(1, 0, LR, 1, None, None, SEED, 0, STEP, 0)
        self.opts_emit = CdOpts(1, 0, LR, 1, self.delta.data_ptr(), None, SEED, 0, STEP, 0)
        self.opts_score = CdOpts(1, 0, 0.0, 0, None, None, SEED, 0, STEP, 3)
        self.mom = Momentum(MU, LAM, self.vel.data_ptr())
        self.rng = Rng(SEED, 0, 4, STEP)
        torch.cuda.synchronize()
        p.arena.freeze_all()

    def call(self, entry, short):
        e, lib, h, B, nv, nh, N = self.e, self.e.lib, self.e.ctx.handle, self.B, self.nv, self.nh, self.N
        P, st, V, H = C.byref(e.params), e._stream(), self.V, self.H
        o, oe, osc, mom, rng = C.byref(self.opts), C.byref(self.opts_emit), C.byref(self.opts_score), C.byref(self.mom), C.byref(self.rng)

        def b(key):
            t = self.buf[key]
            return t.data_ptr(), t.numel() - (16 if key == short else 0)

        ws, wsw, wsb, wsx, m1, m3, pl = b("ws"), b("wsw"), b("wsb"), b("wsx"), b("mir1"), b("mir3"), b("planes")
        vp, out, F, sc = self.vp, self.out, self.F.data_ptr(), self.score.data_ptr()
        calls = {
            "kurbm_cd_step": lambda: lib.kurbm_cd_step(h, P, V.ptr(), B, V.ld, o, 7, *wsw, st),
            "kurbm_cd_step_mom": lambda: lib.kurbm_cd_step_mom(h, P, V.ptr(), B, V.ld, o, 7, *wsw, st, mom),
            "kurbm_cd_step_small": lambda: lib.kurbm_cd_step_small(h, P, V.ptr(), B, V.ld, o, 7, *ws, st),
            "kurbm_cd_epoch": lambda: lib.kurbm_cd_epoch(h, P, V.ptr(), N, V.ld, B, o, *wsw, st),
            "kurbm_cd_epoch_mom": lambda: lib.kurbm_cd_epoch_mom(h, P, V.ptr(), N, V.ld, B, o, *wsw, st, mom),
            "kurbm_cd_epoch_small": lambda: lib.kurbm_cd_epoch_small(h, P, V.ptr(), N, V.ld, B, o, *ws, st),
            "kurbm_cd_epoch_small_scored": lambda: lib.kurbm_cd_epoch_small_scored(h, P, V.ptr(), N, V.ld, B, o, 3, self.host.data_ptr(), *ws, st),
            "kurbm_score_small": lambda: lib.kurbm_score_small(h, P, V.ptr(), B, V.ld, osc, sc, F, *ws, st),
            "kurbm_free_energy": lambda: lib.kurbm_free_energy(h, P, V.ptr(), B, V.ld, F, *ws, st),
            "kurbm_outer_delta": lambda: lib.kurbm_outer_delta(h, V.ptr(), H.ptr(), V.ptr(B), H.ptr(), B, nv, nh, V.ld, H.ld,
                                                               self.dense.data_ptr(), *ws, st),
            "kurbm_bf16_mirror_refresh": lambda: lib.kurbm_bf16_mirror_refresh(h, P, *m1, st),
            "kurbm_x3_mirror_refresh": lambda: lib.kurbm_x3_mirror_refresh(h, P, *m3, st),
            "kurbm_half_step_bf16": lambda: lib.kurbm_half_step_bf16(h, P, *m1, 0, V.ptr(), B, V.ld, 0, 1, rng, out.ptr(), None, None, out.ld, *wsb, st),
            "kurbm_half_step_x3": lambda: lib.kurbm_half_step_x3(h, P, *m3, 0, V.ptr(), 1, B, V.ld, 0, 1, rng, out.ptr(), None, None, out.ld, *wsx, st),
            "kurbm_cd_step_bf16": lambda: lib.kurbm_cd_step_bf16(h, P, *m1, V.ptr(), B, V.ld, o, 7, *wsb, st),
            "kurbm_cd_step_bf16_mom": lambda: lib.kurbm_cd_step_bf16_mom(h, P, *m1, V.ptr(), B, V.ld, o, 7, *wsb, st, mom),
            "kurbm_cd_step_bf16_dp": lambda: lib.kurbm_cd_step_bf16_dp(h, self.comm.handle, P, *m1, V.ptr(), B, V.ld, oe, 0, *wsb, st),
            "kurbm_cd_step_x3": lambda: lib.kurbm_cd_step_x3(h, P, *m3, V.ptr(), vp, B, V.ld, o, 7, *wsx, st),
            "kurbm_cd_step_x3_mom": lambda: lib.kurbm_cd_step_x3_mom(h, P, *m3, V.ptr(), vp, B, V.ld, o, 7, *wsx, st, mom),
            "kurbm_cd_step_x3_dp": lambda: lib.kurbm_cd_step_x3_dp(h, self.comm.handle, P, *m3, V.ptr(), vp, B, V.ld, oe, 0, *wsx, st),
            "kurbm_cd_epoch_x3": lambda: lib.kurbm_cd_epoch_x3(h, P, *m3, V.ptr(), vp, N, V.ld, B, o, *wsx, st),
            "kurbm_cd_epoch_x3_mom": lambda: lib.kurbm_cd_epoch_x3_mom(h, P, *m3, V.ptr(), vp, N, V.ld, B, o, *wsx, st, mom),
            "kurbm_free_energy_x3": lambda: lib.kurbm_free_energy_x3(h, P, *m3, V.ptr(), vp, B, V.ld, F, *wsx, st),
            "kurbm_score_x3": lambda: lib.kurbm_score_x3(h, P, *m3, V.ptr(), vp, B, V.ld, osc, sc, F, *wsx, st),
            "kurbm_x3_dump_plane": lambda: lib.kurbm_x3_dump_plane(h, 0, B, nv, nh, vp, 0, *wsx, out.ptr(), out.ld, st),
            "kurbm_x3_apply_delta": lambda: lib.kurbm_x3_apply_delta(h, P, *m3, self.delta.data_ptr(), LR, 7, st),
            "kurbm_x3_apply_delta_mom": lambda: lib.kurbm_x3_apply_delta_mom(h, P, *m3, self.delta.data_ptr(), LR, 7, st, mom),
            "kurbm_x3_convert_rows": lambda: lib.kurbm_x3_convert_rows(h, V.ptr(), B, V.ld, nv, vp, *pl, st),
        }
        return calls[entry]()


_WS_STEP = ["kurbm_cd_step", "kurbm_cd_step_mom", "kurbm_cd_epoch", "kurbm_cd_epoch_mom"]      # (a wide batch: the query + the header's formula)
_WS_F32 = ["kurbm_cd_step_small", "kurbm_cd_epoch_small", "kurbm_cd_epoch_small_scored", "kurbm_score_small", "kurbm_free_energy",
           "kurbm_outer_delta"]
_BF16 = ["kurbm_half_step_bf16", "kurbm_cd_step_bf16", "kurbm_cd_step_bf16_mom", "kurbm_cd_step_bf16_dp"]
_X3 = ["kurbm_half_step_x3", "kurbm_cd_step_x3", "kurbm_cd_step_x3_mom", "kurbm_cd_step_x3_dp", "kurbm_cd_epoch_x3", "kurbm_cd_epoch_x3_mom",
       "kurbm_free_energy_x3", "kurbm_score_x3"]
REFUSED = ([(e, "wsw") for e in _WS_STEP] + [(e, "ws") for e in _WS_F32] + [(e, "wsb") for e in _BF16] + [(e, "wsx") for e in _X3 + ["kurbm_x3_dump_plane"]]
           + [(e, "mir1") for e in _BF16 + ["kurbm_bf16_mirror_refresh"]]
           + [(e, "mir3") for e in _X3 + ["kurbm_x3_mirror_refresh", "kurbm_x3_apply_delta", "kurbm_x3_apply_delta_mom"]]
           + [("kurbm_x3_convert_rows", "planes")])
_SHORT = {"ws": "workspace", "wsw": "workspace", "wsb": "workspace", "wsx": "workspace", "mir1": "mirror", "mir3": "mirror", "planes": "planes"}


@pytest.fixture(scope="module")
def rig(gpu_device, one_rank_comm):
    return Rig(gpu_device, one_rank_comm)


@gpu
@pytest.mark.parametrize("entry,short", REFUSED, ids=["%s-short_%s" % (e, _SHORT[s]) for e, s in REFUSED])
def test_undersized_buffer_is_refused(rig, entry, short):
    """The queried size minus 16: KURBM_ERR_WORKSPACE, a message, and -- after a synchronise -- an arena in which nothing at all
    has changed: parameters, outputs, scratch, guards."""
    code = rig.call(entry, short)
    msg = rig.e.lib.kurbm_last_error()
    print("%s with %s 16 bytes short: code %d, %r" % (entry, _SHORT[short], code, msg))
    torch.cuda.synchronize()
    try:
        rig.p.arena.check()
    finally:
        rig.p.arena.freeze_all()        # (a call that got through fails its own case, not the ones after it)
    assert code == -4, (entry, short, code, msg)
    assert msg and b"too small" in msg
    assert bool((rig.host == 0).all())


@gpu
def test_full_size_buffers_are_accepted_by_the_same_calls(gpu_device, one_rank_comm):
    """The other half of the refusal test: the very argument lists it uses are valid -- with every size at its query each call
    succeeds, so what was refused there was the size and nothing else."""
    r = Rig(gpu_device, one_rank_comm)
    for b in r.p.arena.bufs:
        b.frozen = None
    for entry in dict.fromkeys(e for e, _ in REFUSED):
        code = r.call(entry, None)
        assert code >= 0, (entry, code, r.e.lib.kurbm_last_error())
    torch.cuda.synchronize()
    r.p.arena.check()
    r.e.check_status()


@gpu
def test_half_step_x3_byte_plane_checks_before_it_enqueues(rig):
    """in_pieces = 1 | KURBM_V_BINARY: a workspace or a mirror 16 bytes short is refused as for the other formats, an unknown
    in_pieces is an argument error, nothing in the arena changes either way -- and the same call at full size succeeds."""
    e, lib = rig.e, rig.e.lib

    def call(in_pieces, short):
        ws, m3 = rig.buf["wsx"], rig.buf["mir3"]
        return lib.kurbm_half_step_x3(e.ctx.handle, C.byref(e.params), m3.data_ptr(), m3.numel() - (16 if short == "mir3" else 0), 0,
                                      rig.V.ptr(), in_pieces, rig.B, rig.V.ld, 0, 1, C.byref(rig.rng), rig.out.ptr(), None, None, rig.out.ld,
                                      ws.data_ptr(), ws.numel() - (16 if short == "wsx" else 0), e._stream())

    for in_pieces, short, want in ((rig.vp, "wsx", -4), (rig.vp, "mir3", -4), (2, None, -1), (3 | 0x10, None, -1), (0x10, None, -1)):
        code = call(in_pieces, short)
        msg = lib.kurbm_last_error()
        torch.cuda.synchronize()
        try:
            rig.p.arena.check()
        finally:
            rig.p.arena.freeze_all()
        assert code == want and msg, (in_pieces, short, code, msg)
        assert (b"too small" in msg) == (want == -4)
    for b in rig.p.arena.bufs:
        b.frozen = None
    try:
        assert call(rig.vp, None) == 0, lib.kurbm_last_error()
        torch.cuda.synchronize()
        rig.p.arena.check()
        e.check_status()
    finally:
        rig.p.arena.freeze_all()


@gpu
def test_size_queries_return_zero_for_non_positive_shapes(gpu_device):
    from keras_unsupervised_amd._lib import Context
    ctx = Context.get(gpu_device.index)
    lib, h = ctx.lib, ctx.handle
    assert lib.kurbm_workspace_bytes(h, 36, 100, 50, 1) > 0 and lib.kurbm_x3_planes_bytes(h, 36, 100, 1) > 0
    for bad in (0, -1):
        for args in ((bad, 100, 50), (36, bad, 50), (36, 100, bad)):
            assert lib.kurbm_workspace_bytes(h, *args, 1) == 0
            assert lib.kurbm_bf16_workspace_bytes(h, *args, 1) == 0
            assert lib.kurbm_x3_workspace_bytes(h, *args, 1, 1) == 0 and lib.kurbm_x3_workspace_bytes(h, *args, 1, 3) == 0
        for args in ((bad, 50), (100, bad)):
            assert lib.kurbm_bf16_mirror_bytes(h, *args) == 0 and lib.kurbm_x3_mirror_bytes(h, *args) == 0
        for args in ((bad, 100), (36, bad)):
            assert lib.kurbm_x3_planes_bytes(h, *args, 1) == 0 and lib.kurbm_x3_planes_bytes(h, *args, 3) == 0 \
                and lib.kurbm_x3_planes_bytes(h, *args, 1 | 0x10) == 0
