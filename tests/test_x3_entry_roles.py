"""The entry of k_gemm_pb (kurbm_x3.hip): the roles part first, and each role maps its block and sets itself up on its own.

Every x3 launch goes through that entry, so what is held here is the whole step, launch by launch, wherever the entry takes another
path: both block mappings (a grid of a multiple of 8 workgroups takes one 2-D block of tiles per XCD, any other grid the linear order),
the dividing path of grids beyond the multiply-high constants (KURBM_MAP_SLOW=1), the linear order on a grid that could take the blocks
(KURBM_X3_XCD2D=0), and a statistics launch of more than one k slice (a loader's first tile reference is a multiply-add on its slice).
Three kinds of data, because their launches walk differently: 0/1 data (the byte-plane walks, whose loaders take their first reference
from the arguments alone), grey levels k / 255 with Bernoulli visibles (the paired walk of the v -> h half step, the transposed
positive statistics) and the same data with Gaussian visibles (the paired walk in the h_neg half step and in the negative statistics).

Shapes (rows, n_vis, n_hid): at least two tiles along m and along n in every launch, a few hundred rows.
  (256, 512, 512)   half steps 2 x 4 = 8 workgroups each way, statistics 2 x 8 tiles x 2 k slices: XCD blocks everywhere
  (384, 300, 130)   half steps 3 x 2 and 3 x 3, statistics 2 x 3 tiles x 3 k slices: the linear order everywhere; partial tiles
"""
import functools

import numpy as np
import pytest
import torch

from oracle import rbm_oracle as O
from oracle.make_golden import synthetic_binary, synthetic_params, synthetic_real
from test_gpu_configs_at_size import STAT_TOL, TOL, _dm, _engine, _split, check_half_step, rel_err, stagewise_cd_check

pytestmark = pytest.mark.gpu

SH_XCD, SH_LIN = (256, 512, 512), (384, 300, 130)
SEED, STEP = 42, 5
# (shape, knobs): the knobs are set on the context for the case and put back to their defaults behind it
CASES = [(SH_XCD, {}), (SH_LIN, {}), (SH_XCD, dict(KURBM_MAP_SLOW=1)), (SH_LIN, dict(KURBM_MAP_SLOW=1)), (SH_XCD, dict(KURBM_X3_XCD2D=0)),
         (SH_XCD, dict(KURBM_BF16_SPLIT=2))]
DEFAULTS = dict(KURBM_MAP_SLOW=0, KURBM_X3_XCD2D=1, KURBM_BF16_SPLIT=-1)
case_id = lambda x: str(x) if isinstance(x, tuple) else (",".join("%s=%d" % kv for kv in x.items()) or "defaults")


@functools.lru_cache(maxsize=None)
def problem(shape, kind):
    """(W, b_h, b_v), v of a shape and a kind of data: made once, shared by every case, never written."""
    rows, nv, nh = shape
    W, b_h, b_v = synthetic_params(nv, nh, seed=5000 + rows)
    if kind == "binary":
        return (W, b_h, b_v), synthetic_binary(rows, nv, seed=5001 + rows, p=0.3)
    if kind == "gauss":
        W = (W * np.float32(4.0)).astype(np.float32)      # pre-activations that cross the relu threshold's (0, 1) range
    return (W, b_h, b_v), (np.floor(synthetic_real(rows, nv, seed=5002 + rows) * 256.0) / 255.0).astype(np.float32)


class knobs_set:
    def __init__(self, dev, knobs):
        from keras_unsupervised_amd._lib import Context
        self.ctx, self.knobs = Context.get(dev.index), knobs

    def __enter__(self):
        for name, value in self.knobs.items():
            self.ctx.set_option(name, value)

    def __exit__(self, *exc):
        for name in self.knobs:
            self.ctx.set_option(name, DEFAULTS[name])


def stagewise_real(e, W, b_h, b_v, v, vd, rows, gauss, seed, step):
    """The x3 step on real-valued data, as test_config2_gaussian_default_mode_stagewise holds it at size: every launch replayed through
    the half-step hooks with the step's own counters and teacher-forced against the oracle, then the fused step's sums against float64
    statistics of those states.  gauss: relu-threshold hidden draws and v_neg ~ N(h.W^T + b_v, 1); else sigmoid and Bernoulli draws."""
    lr = 1e-3 / rows
    rng = O.Rng(seed, step)
    hook = lambda direction, x, act, noise, stream: e.half_step_bf16(direction, x, rows, act, noise, seed, stream, step, pieces=3)
    mode = (O.MODE_VISIBLE_GAUSSIAN,) if gauss else ()
    o = hook("vh", vd, 1 if gauss else 0, 1, O.stream_h(0))
    flips = check_half_step(o, *O.sample_hidden(v, W, b_h, rng, O.stream_h(0), *mode))
    h_pos = o["sample"].to_numpy()
    if gauss:
        o2 = hook("hv", o["sample"], 2, 2, O.stream_v(1))                                # linear mean + N(0, 1)
        loc, _, v1 = O.sample_visible(h_pos, W, b_v, rng, O.stream_v(1), *mode)
        assert np.max(np.abs(o2["prob"].to_numpy() - loc)) <= TOL and np.max(np.abs(o2["sample"].to_numpy() - v1)) <= TOL
    else:
        o2 = hook("hv", o["sample"], 0, 1, O.stream_v(1))
        flips += check_half_step(o2, *O.sample_visible(h_pos, W, b_v, rng, O.stream_v(1)))
    v_neg = o2["sample"].to_numpy()
    h_neg = hook("vh", o2["sample"], 0, 0, 0)["prob"].to_numpy()                         # sigmoid in both modes
    assert np.max(np.abs(h_neg - O.sigmoid(v_neg @ W + b_h))) <= TOL
    assert flips < 64
    e.cd_step(vd, rows, 0, lr, seed, step, apply=False, emit_delta=True, compute="x3", **(dict(mode=mode[0]) if gauss else {}))
    torch.cuda.synchronize()
    nv, nh = W.shape
    dW, dbh, dbv = _split(e.delta_buffer().cpu().numpy().copy(), nv, nh)
    v64, vn64, hp64, hn64 = (a.astype(np.float64) for a in (v, v_neg, h_pos, h_neg))
    ref = v64.T @ hp64 - vn64.T @ hn64
    scale = np.abs(v64).T @ hp64 + np.abs(vn64).T @ hn64 + 1.0                          # the un-cancelled magnitude
    assert np.max(np.abs(dW - ref) / scale) <= 2 * STAT_TOL
    assert np.max(np.abs(lr * dW - lr * ref)) <= TOL
    assert rel_err(dbv, v64.sum(0) - vn64.sum(0)) <= TOL and rel_err(dbh, hp64.sum(0) - hn64.sum(0)) <= TOL


@pytest.mark.parametrize("shape,knobs", CASES, ids=case_id)
def test_binary_data(gpu_device, shape, knobs):
    """0/1 data: the byte-plane walks of the half steps and of the statistics, against the hooks and the oracle; the fused step's
    own planes bit for bit the hooks' states."""
    (W, b_h, b_v), v = problem(shape, "binary")
    with knobs_set(gpu_device, knobs):
        e = _engine(W, b_h, b_v, gpu_device)
        _, _, flips = stagewise_cd_check(e, "x3", W, b_h, b_v, v, _dm(v, gpu_device), shape[0], SEED, STEP)
    assert flips < 64


@pytest.mark.parametrize("shape,knobs", CASES, ids=case_id)
def test_grey_level_data(gpu_device, shape, knobs):
    """Grey levels, Bernoulli visibles: the paired walk in the v -> h half step, the positive statistics as the transposed problem."""
    (W, b_h, b_v), v = problem(shape, "grey")
    with knobs_set(gpu_device, knobs):
        stagewise_real(_engine(W, b_h, b_v, gpu_device), W, b_h, b_v, v, _dm(v, gpu_device), shape[0], False, SEED, STEP)


@pytest.mark.parametrize("shape,knobs", CASES, ids=case_id)
def test_gaussian_visibles(gpu_device, shape, knobs):
    """Grey levels, Gaussian visibles: three-piece planes both ways, the negative statistics on the paired walk."""
    (W, b_h, b_v), v = problem(shape, "gauss")
    with knobs_set(gpu_device, knobs):
        stagewise_real(_engine(W, b_h, b_v, gpu_device), W, b_h, b_v, v, _dm(v, gpu_device), shape[0], True, SEED, STEP)
