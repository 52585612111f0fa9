"""The packed epilogue of the Bernoulli half steps on byte planes (kurbm_x3.hip, "PACKABLE"; knob KURBM_X3_PACKED_EPI).

A 0/1 sample whose every output is a byte plane is kept as packed bytes, four rows of a column per dword, and the column sums, the
transposed plane and the row-major plane are built from those dwords.  The general epilogue (fp32 1.0 / 0.0 per element,
KURBM_X3_PACKED_EPI=0, and whatever a half step with an fp32 output runs) is the reference: same planes, same sums, bit for bit.

Shapes (rows, n_vis, n_hid), the smallest at which this code can go wrong -- the half steps run 128 x 128 tiles here (256 x 64 with
KURBM_X3_TALL=1 where the batch is a whole number of 256-row tiles' halves):
  (256, 64, 64)     one full tile each way
  (200, 100, 72)    a partial row tile; column counts that are no multiple of 64, 16 or 8
  (257, 784, 130)   a row tile holding one row; a column tile holding two columns
  (384, 50, 1024)   a 128-row batch remainder; n_vis below one column tile
"""
import functools

import numpy as np
import pytest
import torch

from oracle.make_golden import synthetic_binary, synthetic_params
from test_gpu_configs_at_size import _dm, _engine, stagewise_cd_check

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64, 64), (200, 100, 72), (257, 784, 130), (384, 50, 1024)]
SEED, STEP = 42, 17
KNOB = "KURBM_X3_PACKED_EPI"


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(W, b_h, b_v), v of a shape: made once, shared by every test, never written."""
    rows, nv, nh = shape
    W0 = synthetic_params(nv, nh, seed=3000 + rows)
    v = synthetic_binary(rows, nv, seed=3001 + rows, p=0.3)
    return W0, v


def _ctx(dev):
    from keras_unsupervised_amd._lib import Context
    return Context.get(dev.index)


def fused_step(dev, shape, fill=0, chain0=None, planes=False):
    """One fused x3 CD-1 step on a fresh engine whose workspace and weight mirror start as `fill` bytes.  Returns the packed delta,
    the decoded planes H_POS, H_POS_T, V_NEG, V_NEG_T, the workspace's bytes and the persistent chain (or None)."""
    from keras_unsupervised_amd import _lib
    W0, v = problem(shape)
    rows = shape[0]
    e = _engine(*W0, dev)
    vd = _dm(v, dev)
    cd = _dm(chain0, dev) if chain0 is not None else None
    ws = e.workspace_bf16(rows, 1, 3, e._x3_pieces(vd, cd, 0))
    if fill:
        ws.fill_(fill)
        e.mirror(3).fill_(fill)
        e._mirrors[3][1] = True        # stale: the library rewrites it from W (pads included) before the step
    pl = e.make_planes(vd, [(0, rows)]) if planes else None
    e.cd_step(vd, rows, 0, 1e-3, SEED, STEP, apply=False, emit_delta=True, compute="x3", v_chain=cd, planes=pl)
    torch.cuda.synchronize()
    delta = e.delta_buffer().cpu().numpy().copy()
    dumped = [e.dump_plane(w, vd, rows).to_numpy() for w in (_lib.PLANE_H_POS, _lib.PLANE_H_POS_T, _lib.PLANE_V_NEG, _lib.PLANE_V_NEG_T)]
    return delta, dumped, ws.cpu().numpy().copy(), (cd.to_numpy() if cd is not None else None)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_stagewise_against_the_hooks_and_the_oracle(gpu_device, shape):
    """The fused step (packed epilogue) against the half-step hooks (fp32 test planes: the general epilogue) and the oracle: u / p /
    samples per half step, the fused step's own planes bit for bit the hooks' states, then the sums."""
    (W, b_h, b_v), v = problem(shape)
    e = _engine(W, b_h, b_v, gpu_device)
    stagewise_cd_check(e, "x3", W, b_h, b_v, v, _dm(v, gpu_device), shape[0], SEED, STEP)


# (KURBM_X3_TALL = 1 runs 256 x 64 tiles only on an even number of 128-row tiles: shapes 1 and 2)
@pytest.mark.parametrize("shape,tall", [(s, -1) for s in SHAPES] + [(s, 1) for s in SHAPES[:2]],
                         ids=lambda x: str(x) if isinstance(x, tuple) else {-1: "tiles_auto", 1: "tiles_256x64"}[x])
def test_packed_and_general_epilogue_leave_the_same_bytes(gpu_device, shape, tall):
    """KURBM_X3_PACKED_EPI = 1 against 0: the four sample planes, the packed delta and every byte of the (zero-initialised) workspace
    -- the planes' paddings, the column partials -- are equal.  (KURBM_X3_TALL = 1: the 256 x 64 instance.)"""
    ctx = _ctx(gpu_device)
    got = []
    try:
        ctx.set_option("KURBM_X3_TALL", tall)
        for packed in (1, 0):
            ctx.set_option(KNOB, packed)
            got.append(fused_step(gpu_device, shape))
    finally:
        ctx.set_option(KNOB, 1)
        ctx.set_option("KURBM_X3_TALL", -1)
    (d1, p1, w1, _), (d0, p0, w0, _) = got
    for name, a, b in zip(("H_POS", "H_POS_T", "V_NEG", "V_NEG_T"), p1, p0):
        assert set(np.unique(b)) <= {0.0, 1.0}
        assert 0.0 < b.mean() < 1.0, "%s: a plane of one value compares nothing" % name
        assert np.array_equal(bits(a), bits(b)), "%s differs between the packed and the general epilogue" % name
    assert np.all(np.isfinite(d0))
    assert np.array_equal(bits(d1), bits(d0)), "the packed delta differs"
    assert np.array_equal(w1, w0), "workspace bytes differ: %d" % int((w1 != w0).sum())


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=str)
def test_padding_is_written_not_assumed(gpu_device, shape):
    """A workspace of 0xFF bytes against a zeroed one: an unwritten zero in the column padding of a row-major plane, or in the rows
    past the batch of a transposed plane, reaches the statistics.  The emitted deltas are equal bit for bit."""
    d0, p0, _, _ = fused_step(gpu_device, shape, fill=0)
    dF, pF, _, _ = fused_step(gpu_device, shape, fill=0xFF)
    assert np.all(np.isfinite(dF))
    assert np.array_equal(bits(dF), bits(d0))
    for a, b in zip(pF, p0):
        assert np.array_equal(bits(a), bits(b))


def test_a_persistent_chain_takes_the_general_epilogue(gpu_device):
    """Path selection at shape 2.  With v_chain the h -> v launch also writes the fp32 chain (out_f32) and the chain's own v -> h launch
    leaves no transposed plane: both run the general epilogue, whatever the knob says, while h_pos stays packed.

    A step with v_chain and a step without cannot be compared plane for plane at the same counters: the chain's hidden states are drawn
    from the chain on stream 64 chain + 32 (kurbm_host_x3.hip, step_chain), not from the data on stream 64 chain + 0, so their v_neg
    are different samples on the parent commit too.  What is held instead: (1) the step with v_chain, every launch replayed through the
    hooks and the oracle (stagewise_cd_check with chain0), its V_NEG planes bit for bit the chain it wrote; (2) that step is
    byte-identical under KURBM_X3_PACKED_EPI = 1 and 0 -- planes, chain, delta; (3) it leaves the same H_POS planes as the step
    without a chain (the one launch the two share on the same counters, packed in both)."""
    from keras_unsupervised_amd import _lib
    shape = SHAPES[1]
    rows = shape[0]
    (W, b_h, b_v), v = problem(shape)
    chain0 = synthetic_binary(rows, shape[1], seed=77, p=0.4)
    e = _engine(W, b_h, b_v, gpu_device)
    vd = _dm(v, gpu_device)
    _, st, _ = stagewise_cd_check(e, "x3", W, b_h, b_v, v, vd, rows, SEED, STEP, chain0=chain0)
    for which in (_lib.PLANE_V_NEG, _lib.PLANE_V_NEG_T):
        assert np.array_equal(e.dump_plane(which, vd, rows).to_numpy(), st["v_neg"])
    for which in (_lib.PLANE_H_POS, _lib.PLANE_H_POS_T):
        assert np.array_equal(e.dump_plane(which, vd, rows).to_numpy(), st["h_pos"])
    ctx = _ctx(gpu_device)
    got = []
    try:
        for packed in (1, 0):
            ctx.set_option(KNOB, packed)
            got.append(fused_step(gpu_device, shape, chain0=chain0))
    finally:
        ctx.set_option(KNOB, 1)
    (d1, p1, w1, c1), (d0, p0, w0, c0) = got
    assert np.array_equal(c1, st["v_neg"]) and np.array_equal(bits(c1), bits(c0))
    assert np.array_equal(bits(d1), bits(d0)) and np.array_equal(w1, w0)
    for a, b in zip(p1, p0):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(p1[2], c1) and np.array_equal(p1[3], c1)
    _, pn, _, _ = fused_step(gpu_device, shape)                      # no chain: h_pos is the same launch on the same counters
    assert np.array_equal(bits(pn[0]), bits(p1[0])) and np.array_equal(bits(pn[1]), bits(p1[1]))


@pytest.mark.parametrize("knobs", [dict(KURBM_X3_F8POS=0), dict(KURBM_X3_BYTES=0), dict(KURBM_X3_F8POS=0, KURBM_X3_BYTES=0)],
                         ids=lambda k: ",".join("%s=%d" % kv for kv in k.items()))
def test_plane_formats_agree(gpu_device, knobs):
    """Shape 2 under the plane-format knobs, as test_config2_x3_plane_formats_agree does at size.  Where a format is outside the packed
    path's condition (bf16 row-major planes with BYTES = 0, a bf16 transposed plane) the launch falls back to the general epilogue,
    and this is the proof.  The chains are bit-identical whatever the format, so both bias sums match to the bit and dW to the
    order of the fp32 additions in the statistics GEMM."""
    shape = SHAPES[1]
    nv, nh = shape[1], shape[2]
    ctx = _ctx(gpu_device)
    got = []
    try:
        for kn in ({}, knobs):
            for name, value in kn.items():
                ctx.set_option(name, value)
            d, planes, _, _ = fused_step(gpu_device, shape, planes=True)
            got.append((d[: nv * nh].reshape(nv, nh), d[nv * nh: nv * nh + nh], d[nv * nh + nh:], planes))
    finally:
        for name in knobs:
            ctx.set_option(name, 1)
    (dW0, dbh0, dbv0, p0), (dW1, dbh1, dbv1, p1) = got
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)                                     # the decoded 0/1 planes: the same states
    assert np.array_equal(dbv0, dbv1)
    assert np.array_equal(dbh0, dbh1)
    assert np.max(np.abs(dW0 - dW1)) <= 2e-6 * max(1.0, float(np.abs(dW1).max()))
