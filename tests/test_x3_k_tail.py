"""The last k-tile of an x3 half step on a byte plane (kurbm_x3.hip, the TAIL tile; knob KURBM_X3_KTAIL).

A half step walks K = round_up(n, 64) in k-tiles of two k-steps of 32.  Where round_up(n, 32) < round_up(n, 64) the second k-step of the
last tile lies wholly in the k padding -- zeros in both operands -- and the byte-plane walk does not multiply it.  The products left out
are 0 * w into accumulators that started at +0, so every plane, sum and workspace byte stays what KURBM_X3_KTAIL=0 (the whole tile)
leaves, bit for bit.

Shapes (rows, n_vis, n_hid), the smallest at which the tail can go wrong; v -> h has k = n_vis, h -> v has k = n_hid:
  (256, 80, 64)     tail skipped in v -> h (80 -> 96 < 128); h -> v walks one whole tile
  (200, 96, 72)     exactly one real k-step in the last tile, the boundary: skipped (and 72 -> 96 < 128: in h -> v too)
  (256, 97, 64)     33 real k in the last tile: not skipped
  (256, 16, 64)     the only tile is a half tile (the tail tile is entered straight from the prologue)
  (256, 128, 80)    tail in h -> v only
  (257, 784, 130)   the flagship's k (13 tiles) with partial row and column tiles; h -> v: 130 -> 160 < 192, three tiles
The tail tile is the second of its 128-deep A block in the two-tile walks above (tile 1) and the first of a block here (tiles 12, 2).
"""
import functools

import numpy as np
import pytest
import torch

from oracle.make_golden import synthetic_binary, synthetic_params
from test_gpu_configs_at_size import _dm, _engine, stagewise_cd_check

pytestmark = pytest.mark.gpu

SHAPES = [(256, 80, 64), (200, 96, 72), (256, 97, 64), (256, 16, 64), (256, 128, 80), (257, 784, 130)]
SEED, STEP = 42, 23
KNOB = "KURBM_X3_KTAIL"
PLANE_NAMES = ("H_POS", "H_POS_T", "V_NEG", "V_NEG_T")


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(W, b_h, b_v), v of a shape: made once, shared by every test, never written."""
    rows, nv, nh = shape
    return synthetic_params(nv, nh, seed=4000 + rows + nv), synthetic_binary(rows, nv, seed=4001 + rows + nv, p=0.3)


def _ctx(dev):
    from keras_unsupervised_amd._lib import Context
    return Context.get(dev.index)


def fused_step(dev, shape, fill=0):
    """One fused x3 CD-1 step on a fresh engine whose workspace and weight mirror start as `fill` bytes.  Returns the packed delta,
    the decoded planes H_POS, H_POS_T, V_NEG, V_NEG_T and the workspace's bytes."""
    from keras_unsupervised_amd import _lib
    W0, v = problem(shape)
    rows = shape[0]
    e = _engine(*W0, dev)
    vd = _dm(v, dev)
    ws = e.workspace_bf16(rows, 1, 3, e._x3_pieces(vd, None, 0))
    if fill:
        ws.fill_(fill)
        e.mirror(3).fill_(fill)
        e._mirrors[3][1] = True        # stale: the library rewrites it from W (pads included) before the step
    e.cd_step(vd, rows, 0, 1e-3, SEED, STEP, apply=False, emit_delta=True, compute="x3")
    torch.cuda.synchronize()
    delta = e.delta_buffer().cpu().numpy().copy()
    dumped = [e.dump_plane(w, vd, rows).to_numpy() for w in (_lib.PLANE_H_POS, _lib.PLANE_H_POS_T, _lib.PLANE_V_NEG, _lib.PLANE_V_NEG_T)]
    return delta, dumped, ws.cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_stagewise_against_the_hooks_and_the_oracle(gpu_device, shape):
    """The fused step (tail tiles where the shape has them) against the half-step hooks and the oracle: u / p / samples per half
    step, the fused step's own planes bit for bit the hooks' states, then the sums."""
    (W, b_h, b_v), v = problem(shape)
    e = _engine(W, b_h, b_v, gpu_device)
    stagewise_cd_check(e, "x3", W, b_h, b_v, v, _dm(v, gpu_device), shape[0], SEED, STEP)


# (KURBM_X3_TALL = 1 runs the 256 x 64 instance -- the flagship's -- only on an even number of 128-row tiles: all shapes but the last)
@pytest.mark.parametrize("shape,tall", [(s, -1) for s in SHAPES] + [(s, 1) for s in SHAPES[:5]],
                         ids=lambda x: str(x) if isinstance(x, tuple) else {-1: "tiles_auto", 1: "tiles_256x64"}[x])
def test_tail_and_whole_tile_leave_the_same_bytes(gpu_device, shape, tall):
    """KURBM_X3_KTAIL = 1 against 0: the four sample planes, the packed delta and every byte of the (zero-initialised) workspace are
    equal."""
    ctx = _ctx(gpu_device)
    got = []
    try:
        ctx.set_option("KURBM_X3_TALL", tall)
        for tail in (1, 0):
            ctx.set_option(KNOB, tail)
            got.append(fused_step(gpu_device, shape))
    finally:
        ctx.set_option(KNOB, 1)
        ctx.set_option("KURBM_X3_TALL", -1)
    (d1, p1, w1), (d0, p0, w0) = got
    for name, a, b in zip(PLANE_NAMES, p1, p0):
        assert set(np.unique(b)) <= {0.0, 1.0}
        assert 0.0 < b.mean() < 1.0, "%s: a plane of one value compares nothing" % name
        assert np.array_equal(bits(a), bits(b)), "%s differs between the tail tile and the whole tile" % name
    assert np.all(np.isfinite(d0))
    assert np.array_equal(bits(d1), bits(d0)), "the packed delta differs"
    assert np.array_equal(w1, w0), "workspace bytes differ: %d" % int((w1 != w0).sum())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_skip_reads_nothing_the_step_does_not_write(gpu_device, shape):
    """A workspace (and mirror) of 0xFF bytes against zeroed ones: the planes and the emitted delta are equal bit for bit -- neither
    the tail tile nor the k-steps beside it depend on a byte that the step itself does not write."""
    d0, p0, _ = fused_step(gpu_device, shape, fill=0)
    dF, pF, _ = fused_step(gpu_device, shape, fill=0xFF)
    assert np.all(np.isfinite(dF))
    assert np.array_equal(bits(dF), bits(d0))
    for name, a, b in zip(PLANE_NAMES, pF, p0):
        assert np.array_equal(bits(a), bits(b)), name
