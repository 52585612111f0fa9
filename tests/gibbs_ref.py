"""A float64 numpy restatement of the Gibbs run of include/kurbm.h (kurbm_gibbs_run), drawing with oracle.philox -- the yardstick
of tests/test_gpu_gibbs.py, and of the CPU tier's check (tests/test_gibbs_host.py) that the yardstick itself samples p(v).

    v_0 = v_init;   sweep t = 1 .. T,  T = burn_in + (n_keep - 1) thin:
        h_t = [u < act_h(v_{t-1}.W + b_h)]                       act_h = sigmoid (Bernoulli visibles) / relu (Gaussian visibles)
        v_t = [u < sigmoid(h_t.W^T + b_v)]   or   (h_t.W^T + b_v) + z   (Gaussian visibles)
        v_t[:, c] = v_init[:, c] for every clamped c
    kept sample j = v_{burn_in + j thin};  prob = the sigmoid / the mean it was drawn from (clamped columns: v_init).

Draws: row = chain0 + chain, col = unit, step = t; sites GIBBS_H and GIBBS_V (normals: that plane and | 0x80000000).
"""
import functools

import numpy as np

from oracle import philox

STREAM_GIBBS_H, STREAM_GIBBS_V = 0x210, 0x211
MODE_BERNOULLI, MODE_GAUSSIAN = 0, 1
TOL = 1e-4          # the project's fp32 bar (tests/test_gpu_parity.py)
FLIP_BAND = 1e-5    # |u - p| below which a sample may legitimately differ


def f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def uniform(rows, cols, seed, stream, step, chain0):
    return philox.uniform(rows, cols, seed, stream, step, row0=chain0).astype(np.float64)


def mask_of(clamp, n_vis):
    m = np.zeros(n_vis, dtype=bool)
    if clamp is not None:
        c = np.asarray(clamp)
        if c.dtype == np.bool_:
            m |= c
        else:
            m[c.astype(np.int64)] = True
    return m


def sweep(W, b_h, b_v, v, t, chain0, seed, mode):
    """One unclamped sweep from v: (h, p_h, u_h, v_new, p_v, near) -- near[chain]: some Bernoulli draw of the sweep fell inside
    FLIP_BAND of its probability."""
    W, b_h, b_v, v = f64(W, b_h, b_v, v)
    n, (nv, nh) = v.shape[0], W.shape
    x = v @ W + b_h
    ph = np.maximum(x, 0.0) if mode == MODE_GAUSSIAN else sigmoid(x)
    uh = uniform(n, nh, seed, STREAM_GIBBS_H, t, chain0)
    h = (uh < ph).astype(np.float64)
    near = (np.abs(uh - ph) <= FLIP_BAND).any(axis=1)
    y = h @ W.T + b_v
    if mode == MODE_GAUSSIAN:
        pv = y
        vn = y + philox.normal(n, nv, seed, STREAM_GIBBS_V, t, row0=chain0).astype(np.float64)
    else:
        pv = sigmoid(y)
        uv = uniform(n, nv, seed, STREAM_GIBBS_V, t, chain0)
        vn = (uv < pv).astype(np.float64)
        near |= (np.abs(uv - pv) <= FLIP_BAND).any(axis=1)
    return h, ph, uh, vn, pv, near


def run(W, b_h, b_v, v_init, chain0, seed, mode=MODE_BERNOULLI, burn_in=1, thin=1, n_keep=1, clamp=None):
    """The whole run: (v_kept [n_keep, n_chains, n_vis], prob_kept likewise, flagged [n_chains] -- some hidden or
    Bernoulli-visible draw of the chain fell inside FLIP_BAND of its probability, so an fp32 evaluation may legitimately take
    the other branch there and part from this chain)."""
    v0 = np.asarray(v_init, dtype=np.float64)
    n, nv = v0.shape
    m = mask_of(clamp, nv)
    T = burn_in + (n_keep - 1) * thin
    v = v0.copy()
    flagged = np.zeros(n, dtype=bool)
    vs, ps = [], []
    for t in range(1, T + 1):
        _, _, _, v, pv, near = sweep(W, b_h, b_v, v, t, chain0, seed, mode)
        flagged |= near
        v[:, m] = v0[:, m]
        if t >= burn_in and (t - burn_in) % thin == 0:
            pv = pv.copy()
            pv[:, m] = v0[:, m]
            vs.append(v.copy())
            ps.append(pv)
    return np.stack(vs), np.stack(ps), flagged


# ---- exact distributions of a small Bernoulli RBM (enumeration) -------------------------------------------------------------
def state_matrix(n):
    """All 2^n states, bit i of the state's index = unit i."""
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)


def state_index(v):
    v = np.asarray(v)
    return (v.astype(np.int64) << np.arange(v.shape[1])[None, :]).sum(axis=1)


def exact_pv(W, b_h, b_v, clamp=None, values=None):
    """p(v) over all 2^n_vis states (index = state_index); with clamp / values: p(v | v[clamp] = values), zero elsewhere."""
    W, b_h, b_v = f64(W, b_h, b_v)
    S = state_matrix(W.shape[0])
    e = S @ b_v + np.logaddexp(0.0, S @ W + b_h).sum(axis=1)
    if clamp is not None:
        ok = (S[:, np.asarray(clamp)] == np.asarray(values, dtype=np.float64)[None, :]).all(axis=1)
        e = np.where(ok, e, -np.inf)
    p = np.exp(e - e.max())
    return p / p.sum()


def band_violations(samples, p, sigmas):
    """Indices of the states whose empirical frequency f over the rows of `samples` misses |f - p| <= sigmas sqrt(p (1 - p) / N)
    + 1 / N, and the frequencies."""
    N = samples.shape[0]
    f = np.bincount(state_index(samples), minlength=p.size) / float(N)
    bad = np.abs(f - p) > sigmas * np.sqrt(p * (1.0 - p) / N) + 1.0 / N
    return np.nonzero(bad)[0], f


# ---- the models of the tests (shared by the GPU and the CPU tier; computed once per process) --------------------------------
def normal_params(seed, n_vis, n_hid, w_std, b_std):
    """W, then b_h, b_v, in that order, from default_rng(seed); fp32 values."""
    g = np.random.default_rng(seed)
    W = g.normal(0.0, w_std, (n_vis, n_hid)).astype(np.float32)
    b_h = g.normal(0.0, b_std, n_hid).astype(np.float32)
    b_v = g.normal(0.0, b_std, n_vis).astype(np.float32)
    return W, b_h, b_v


FREE_CHAINS, FREE_SHAPE, FREE_SWEEPS = 200, (70, 36), 8
CLAMP_COLS = np.array([0, 5, 63, 64, 69])          # both sides of the 64-group boundary of a k-permuted byte plane
GAUSS_SWEEPS = 4
DIST_SHAPE, DIST_CHAINS, DIST_BURN = (6, 5), 8192, 200
DIST_CLAMP, DIST_VALUES = np.array([0, 3]), np.array([1.0, 0.0])


def free_params(seed):
    return normal_params(300 + seed, FREE_SHAPE[0], FREE_SHAPE[1], 0.3, 0.3)


def free_init(seed):
    return (np.random.default_rng(400 + seed).random((FREE_CHAINS, FREE_SHAPE[0])) < 0.5).astype(np.float32)


def gauss_init(seed):
    return np.random.default_rng(500 + seed).normal(0.0, 1.0, (FREE_CHAINS, FREE_SHAPE[0])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def free_run(seed, burn_in=FREE_SWEEPS, thin=1, n_keep=1, clamped=False):
    """Restatement of the short Bernoulli run (200 chains, 70 x 36) for `seed`."""
    W, b_h, b_v = free_params(seed)
    return run(W, b_h, b_v, free_init(seed), 0, seed, MODE_BERNOULLI, burn_in, thin, n_keep, CLAMP_COLS if clamped else None)


def gauss_params(seed):
    return normal_params(300 + seed, FREE_SHAPE[0], FREE_SHAPE[1], 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def gauss_run(seed, clamped=False):
    """Restatement of the short Gaussian run (200 chains, 70 x 36, four sweeps, real-valued start)."""
    W, b_h, b_v = gauss_params(seed)
    return run(W, b_h, b_v, gauss_init(seed), 0, seed, MODE_GAUSSIAN, GAUSS_SWEEPS, 1, 1, CLAMP_COLS if clamped else None)


def dist_params():
    return normal_params(77, DIST_SHAPE[0], DIST_SHAPE[1], 0.6, 0.4)


def dist_init(clamped):
    v = (np.random.default_rng(78).random((DIST_CHAINS, DIST_SHAPE[0])) < 0.5).astype(np.float32)
    if clamped:
        v[:, DIST_CLAMP] = DIST_VALUES.astype(np.float32)[None, :]
    return v


@functools.lru_cache(maxsize=None)
def dist_run(clamped, seed=5):
    """Restatement of the distribution test: 6 x 5, 8192 chains, 200 sweeps, one kept sample."""
    W, b_h, b_v = dist_params()
    v, _, _ = run(W, b_h, b_v, dist_init(clamped), 0, seed, MODE_BERNOULLI, DIST_BURN, 1, 1, DIST_CLAMP if clamped else None)
    return v[0]
