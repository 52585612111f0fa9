"""GPU tier of the lattice tests: every linear GEMM hook held to exact arithmetic, bit for bit (fixtures and the argument why
exactness is the only right answer: tests/lattice.py; its CPU tier: tests/test_lattice_host.py).

Every comparison is np.array_equal on the uint32 views of the kernel's fp32 output and of the float64 result cast to fp32 -- no
tolerance anywhere.  ACT_LINEAR with NOISE_NONE, plus ACT_RELU cases (a sign error cannot hide behind a symmetric fixture) and,
for the x3 h -> v direction, the mean plane of an ACT_LINEAR + NOISE_GAUSSIAN half step.

what                         hook                                   swept
---------------------------  -------------------------------------  ------------------------------------------------------------
fp32 MFMA half steps         kurbm_half_step_{vh,hv}_dbg            KURBM_CFG_VH / _HV 0 .. 7 and the planner's choice; a row window
                                                                    into a wider matrix with a wide leading dimension
x3 half steps                kurbm_half_step_x3, in_pieces          KURBM_X3_TALL 0 1, _PAIR 0, _BYTES 0, _MFAST 0, _XCD2D 0,
                             1 | KURBM_V_BINARY (bytes), 1, 3       KURBM_MAP_SLOW 1 one at a time from the default, TALL x PAIR
rounded-bf16 half steps      kurbm_half_step_bf16                   KURBM_X3_TALL 0 1, _MFAST 0, _XCD2D 0, KURBM_MAP_SLOW 1
fp32 statistics              kurbm_outer_delta                      KURBM_CFG_OUTER 0 .. 7, KURBM_SPLIT 1 2 3 5, KURBM_TILE_MAJOR 0
mirror after an update       kurbm_x3_apply_delta (+ _mom),         W, biases, velocity and the half steps of both directions on the
                             kurbm_apply_delta (+ _mom) + refresh   updated mirror

Shapes (rows, n_vis, n_hid): lattice.SHAPES.  Out of scope (README): the x3 statistics GEMM on real-valued planes (no hook injects
planes), the one-launch small step, the AIS, label and class-gradient kernels (no linear outputs), KURBM_X3_FULL.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice as L

pytestmark = pytest.mark.gpu


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


SHAPE_IDS = list(L.SHAPES)
DEFAULTS = {"KURBM_X3_TALL": -1, "KURBM_X3_PAIR": 1, "KURBM_X3_BYTES": 1, "KURBM_X3_MFAST": 1, "KURBM_X3_XCD2D": 1, "KURBM_MAP_SLOW": 0,
            "KURBM_CFG_VH": -1, "KURBM_CFG_HV": -1, "KURBM_CFG_OUTER": -1, "KURBM_SPLIT": -1, "KURBM_TILE_MAJOR": 1}
# one knob at a time from the default (a value equal to the default IS the default case), then TALL x PAIR jointly
X3_KNOBS = [{}, {"KURBM_X3_TALL": 0}, {"KURBM_X3_TALL": 1}, {"KURBM_X3_PAIR": 0}, {"KURBM_X3_BYTES": 0}, {"KURBM_X3_MFAST": 0},
            {"KURBM_X3_XCD2D": 0}, {"KURBM_MAP_SLOW": 1}, {"KURBM_X3_TALL": 0, "KURBM_X3_PAIR": 0}, {"KURBM_X3_TALL": 1, "KURBM_X3_PAIR": 0}]
BF16_KNOBS = [{}, {"KURBM_X3_TALL": 0}, {"KURBM_X3_TALL": 1}, {"KURBM_X3_MFAST": 0}, {"KURBM_X3_XCD2D": 0}, {"KURBM_MAP_SLOW": 1}]
# (input format, fixture): bytes = the new hook format; 'x3' on the 0/1 'sparse' data is forced three pieces: legal and exact
X3_FIXTURES = [("bytes", "sparse"), ("bytes", "deep"), ("bytes", "dense"), ("bf16", "R3"), ("x3", "R1"), ("x3", "R2"), ("x3", "sparse")]
F32_FIXTURES = ["sparse", "deep", "dense", "R2"]       # R2: real-valued, bits_a + bits_b = 20
BF16_FIXTURES = [("b8", "b8"), ("b8", "b8n")]


def knob_id(k):
    return "default" if not k else "+".join("%s=%d" % (n.replace("KURBM_", ""), v) for n, v in k.items())


def set_knobs(ctx_option, knobs):
    for name, value in knobs.items():
        ctx_option(name, value, DEFAULTS[name])


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def dm(x, dev, pad=0):
    """DeviceMatrix of host array x; pad > 0: a leading dimension `pad` floats beyond round_up(cols, 4), padding NaN."""
    from keras_unsupervised_amd.ebm.engine import DeviceMatrix, round_up
    if not pad:
        return DeviceMatrix.from_host(x, dev)
    rows, cols = x.shape
    ld = round_up(cols, 4) + pad
    t = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=dev)
    t[:, :cols].copy_(torch.from_numpy(np.ascontiguousarray(x, np.float32)))
    return DeviceMatrix(t, rows, cols, ld)


@pytest.fixture(scope="module")
def rbms(gpu_device):
    """(Problem, DeviceRBM) per (weights, data kind, shape), made once: the weights, mirrors and workspaces depend on none of the
    knobs swept here."""
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    cache = {}

    def get(kind, shape, data_kind=None):
        key = (kind, data_kind, shape)
        if key not in cache:
            p = L.Problem(kind, L.SHAPES[shape], data_kind=data_kind)
            cache[key] = (p, DeviceRBM(*p.params(), gpu_device))
        return cache[key]

    return get


class Tally:
    """Collects every mismatch of a case (one GPU run should say all it can) and counts what was compared."""

    def __init__(self):
        self.fails, self.outputs, self.calls = [], 0, 0

    def eq(self, got, ref, what):
        got = got.to_numpy() if hasattr(got, "to_numpy") else got
        assert got.shape == ref.shape, what
        bad = bits(got) != bits(ref)
        self.outputs += ref.size
        self.calls += 1
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            self.fails.append("%s: %d of %d outputs differ (rows %d, columns %d touched); first at %s: got %r, exact %r"
                              % (what, int(bad.sum()), bad.size, int(bad.any(axis=1).sum()), int(bad.any(axis=0).sum()), i,
                                 float(got[i]), float(ref[i])))

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def x3_plan(shape, fixtures=X3_FIXTURES):
    """The calls of one x3 / rounded-bf16 case: (format, kind, direction, call, act, noise) -- every (format, fixture) in both
    directions over the calls that walk every k, ACT_LINEAR; the first fixture of each format also ACT_RELU (v -> h) and, h -> v,
    ACT_LINEAR + NOISE_GAUSSIAN (the mean plane)."""
    from keras_unsupervised_amd._lib import ACT_LINEAR, ACT_RELU, NOISE_GAUSSIAN, NOISE_NONE
    plan, seen = [], set()
    for fmt, kind in fixtures:
        p = L.Problem(kind if fmt != "b8" else "b8", L.SHAPES[shape], data_kind=kind if fmt == "b8" else None)
        for direction in ("vh", "hv"):
            for call in range(p.calls(direction)):
                plan.append((fmt, kind, direction, call, ACT_LINEAR, NOISE_NONE))
        if fmt not in seen:
            seen.add(fmt)
            plan.append((fmt, kind, "vh", 0, ACT_RELU, NOISE_NONE))
            plan.append((fmt, kind, "hv", 0, ACT_LINEAR, NOISE_GAUSSIAN))
    return plan


def run_half_steps_bf16(rbms, dev, shape, plan, pieces, tally, tag):
    from keras_unsupervised_amd._lib import ACT_RELU
    for fmt, kind, direction, call, act, noise in plan:
        p, e = rbms("b8", shape, kind) if pieces == 1 else rbms(kind, shape)
        fx = p.fixture(direction, call)
        out = e.half_step_bf16(direction, dm(fx.a, dev), p.rows, act, noise, 7, 0x10, 1, pieces=pieces, want_prob=True, want_u=False,
                               in_format=fmt if pieces == 3 else None)
        tally.eq(out["prob"], fx.ref(relu=act == ACT_RELU), "%s %s %s/%s %s call %d act %d noise %d" % (tag, shape, fmt, kind, direction, call, act, noise))


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("knobs", X3_KNOBS, ids=knob_id)
def test_x3_half_steps_are_exact(gpu_device, ctx_option, rbms, knobs, shape):
    """kurbm_half_step_x3 on the lattice: the byte plane (k_gemm_pb<..., AB>, the production half step of every 0/1 chain, reached
    on its own only through in_pieces = 1 | KURBM_V_BINARY), one bf16 piece and three pieces (the paired walk, or with
    KURBM_X3_PAIR=0 the three segments in turn), against the three-piece mirror in both orientations."""
    set_knobs(ctx_option, knobs)
    t = Tally()
    run_half_steps_bf16(rbms, gpu_device, shape, x3_plan(shape), 3, t, "x3 " + knob_id(knobs))
    torch.cuda.synchronize()
    t.done()


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("knobs", BF16_KNOBS, ids=knob_id)
def test_rounded_bf16_half_steps_are_exact_on_bf16_weights(gpu_device, ctx_option, rbms, knobs, shape):
    """kurbm_half_step_bf16 (operands ROUNDED to bf16) on weights and data that are exactly bf16: rounding changes nothing, so the
    same bitwise bar holds -- 0/1 data and dense 4-bit data."""
    set_knobs(ctx_option, knobs)
    t = Tally()
    run_half_steps_bf16(rbms, gpu_device, shape, x3_plan(shape, [("b8", "b8"), ("b8", "b8n")]), 1, t, "bf16 " + knob_id(knobs))
    t.done()


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("cfg", [-1] + list(range(8)), ids=lambda c: "auto" if c < 0 else "cfg%d" % c)
def test_fp32_half_steps_are_exact(gpu_device, ctx_option, rbms, cfg, shape):
    """The fp32 MFMA half steps at each of the eight tile configurations (and the planner's choice): sparse, deep, dense and one
    real-valued fixture, both directions; ACT_RELU; a window of rows (row_start > 0) of a matrix with a wide, NaN-padded leading
    dimension."""
    from keras_unsupervised_amd._lib import ACT_LINEAR, ACT_RELU, NOISE_NONE
    set_knobs(ctx_option, {"KURBM_CFG_VH": cfg, "KURBM_CFG_HV": cfg})
    t = Tally()
    tag = "fp32 cfg %d %s" % (cfg, shape)

    def half(e, direction, x, rows, row_start, act):
        return e.half_step(direction, x, rows, row_start, act, NOISE_NONE, 7, 0x10, 1, want_sample=False, want_prob=True)["prob"]

    for kind in F32_FIXTURES:
        p, e = rbms(kind, shape)
        for direction in ("vh", "hv"):
            for call in range(p.calls(direction)):
                fx = p.fixture(direction, call)
                t.eq(half(e, direction, dm(fx.a, gpu_device), p.rows, 0, ACT_LINEAR), fx.ref(), "%s %s %s call %d" % (tag, kind, direction, call))
        fx = p.fixture("vh")
        t.eq(half(e, "vh", dm(fx.a, gpu_device), p.rows, 0, ACT_RELU), fx.ref(relu=True), "%s %s vh relu" % (tag, kind))
    p, e = rbms("sparse", shape)
    for direction in ("vh", "hv"):
        fx = p.fixture(direction, 0, rows=p.rows + 3)
        got = half(e, direction, dm(fx.a, gpu_device, pad=8), p.rows, 3, ACT_LINEAR)
        t.eq(got, fx.ref()[3:], "%s sparse %s rows 3.. of a wide matrix" % (tag, direction))
    t.done()


STATS = ([{}] + [{"KURBM_CFG_OUTER": c} for c in range(8)] + [{"KURBM_SPLIT": s} for s in (1, 2, 3, 5)] + [{"KURBM_TILE_MAJOR": 0}])


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("knobs", STATS, ids=knob_id)
def test_fp32_statistics_are_exact(gpu_device, ctx_option, knobs, shape):
    """kurbm_outer_delta, dW = v_pos^T h_pos - v_neg^T h_neg with k = the batch, all four planes on the lattice (0/1 visibles, and
    visibles of up to 6 bits; hiddens of 8 bits): every tile configuration, split-K 1 2 3 5 (any slicing sums to the same
    bits), both slab orders."""
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    set_knobs(ctx_option, knobs)
    rows, nv, nh = L.SHAPES[shape]
    e = DeviceRBM(np.zeros((nv, nh), np.float32), np.zeros(nh, np.float32), np.zeros(nv, np.float32), gpu_device)
    t = Tally()
    for kind in ("binary", "six"):
        fx, planes = L.stats_problem(kind, L.SHAPES[shape])
        vp, hp, vn, hn = (dm(x, gpu_device) for x in planes)
        got = e.outer_delta(vp, hp, vn, hn, rows)
        t.eq(got.cpu().numpy(), fx.ref(), "stats %s %s %s" % (knob_id(knobs), shape, kind))
    t.done()


UPDATES = [("x3", False), ("x3", True), ("bf16", False), ("bf16", True)]


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("compute,mom", UPDATES, ids=["%s%s" % (c, "-mom" if m else "") for c, m in UPDATES])
def test_mirror_after_an_update_is_exact(gpu_device, compute, mom, shape):
    """W' = W + lr dW with everything on the lattice (lr = 2^-3; momentum 0.5 on an even velocity): kurbm_x3_apply_delta[_mom]
    rewrites the three-piece mirror in the same launch (two launches where n_hid % 4 != 0: shape 'mid'), the rounded-bf16 path
    applies with kurbm_apply_delta[_mom] and refreshes.  The master weights, biases and velocity equal the exact update, and the
    half steps of both directions ON THE UPDATED MIRROR equal the exact product with the updated weights -- a piece left stale by
    the rewrite changes most of these outputs (tests/test_lattice_host.py)."""
    from keras_unsupervised_amd._lib import ACT_LINEAR, NOISE_NONE
    from keras_unsupervised_amd.ebm.engine import DeviceRBM
    pieces = 3 if compute == "x3" else 1
    up = L.UpdateProblem("sparse" if pieces == 3 else "b8", L.SHAPES[shape])
    rows = L.SHAPES[shape][0]
    e = DeviceRBM(*up.params(), gpu_device)
    t = Tally()

    def half_steps(updated, tag):
        for direction in ("vh", "hv"):
            fx = up.fixture(direction, mom, updated=updated)
            for fmt in (("bytes", "x3") if pieces == 3 else (None,)):
                out = e.half_step_bf16(direction, dm(fx.a, gpu_device), rows, ACT_LINEAR, NOISE_NONE, 7, 0x10, 1, pieces=pieces, want_u=False,
                                       in_format=fmt)
                t.eq(out["prob"], fx.ref(), "update %s%s %s %s %s %s" % (compute, "-mom" if mom else "", shape, tag, direction, fmt))

    half_steps(False, "before")                      # (makes the mirror the update has to rewrite)
    e.delta_buffer().copy_(torch.from_numpy(up.delta()))
    if mom:
        e.set_velocity(*up.velocity())
    e.apply_delta(up.LR, compute=compute, momentum=(up.MU, 0.0) if mom else None)
    Wi, bhi, bvi, vwi, vhi, vvi = up.after(mom)
    W, b_h, b_v = e.get_weights()
    for got, want, name in ((W, Wi, "W"), (b_h, bhi, "b_h"), (b_v, bvi, "b_v")):
        t.eq(got, up._f(want), "update %s %s: %s" % (compute, shape, name))
    if mom:
        for got, want, name in zip(e.get_velocity(), (vwi, vhi, vvi), ("vel_W", "vel_b_h", "vel_b_v")):
            t.eq(got, up._f(want), "update %s %s: %s" % (compute, shape, name))
    half_steps(True, "after")
    t.done()
