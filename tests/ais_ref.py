"""A float64 numpy restatement of the AIS chain of include/kurbm.h (kurbm_ais_run), drawing with oracle.philox -- the yardstick of
tests/test_gpu_ais.py, and of the CPU tier's check (tests/test_ais_host.py) that the yardstick itself estimates log Z.

    p*_beta(v) = exp((1 - beta) b_A.v + beta b_v.v) prod_j (1 + exp(beta a_j)),   a = v.W + b_h
    v_0 = [u < sigmoid(b_A)];   for k = 1 .. K:
        Delta_k = (beta_k - beta_{k-1}) (b_v - b_A).v_{k-1} + sum_j [softplus(beta_k a_j) - softplus(beta_{k-1} a_j)]
        h = [u < sigmoid(beta_k a)];   v_k = [u < sigmoid((1 - beta_k) b_A + beta_k (h.W^T + b_v))]
    log w = sum_k Delta_k

Draws: row = chain0 + chain, col = unit, step = k; sites AIS_INIT (step 0), AIS_H, AIS_V.
"""
import functools

import numpy as np

from oracle import philox

STREAM_AIS_INIT, STREAM_AIS_H, STREAM_AIS_V = 0x200, 0x201, 0x202
TOL = 1e-4          # the project's fp32 bar (tests/test_gpu_parity.py)
FLIP_BAND = 1e-5    # |u - p| below which a sample may legitimately differ


def f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def uniform(rows, cols, seed, stream, step, chain0):
    return philox.uniform(rows, cols, seed, stream, step, row0=chain0).astype(np.float64)


def delta(W, b_h, b_v, b_a, beta_prev, beta, v):
    """(Delta_k per chain, the un-cancelled magnitude sum_j |term_j| + |dbeta| sum_i |(b_v - b_A)_i v_i| per chain)."""
    W, b_h, b_v, b_a, v = f64(W, b_h, b_v, b_a, v)
    a = v @ W + b_h
    terms = softplus(beta * a) - softplus(beta_prev * a)
    db = beta - beta_prev
    d = b_v - b_a
    return db * (v @ d) + terms.sum(axis=1), np.abs(terms).sum(axis=1) + abs(db) * (v @ np.abs(d))


def hidden(W, b_h, beta, k, v, chain0, seed):
    """(p, u, h) of the hidden site of temperature k."""
    W, b_h, v = f64(W, b_h, v)
    p = sigmoid(beta * (v @ W + b_h))
    u = uniform(v.shape[0], W.shape[1], seed, STREAM_AIS_H, k, chain0)
    return p, u, (u < p).astype(np.float64)


def visible(W, b_v, b_a, beta, k, h, chain0, seed):
    """(p, u, v) of the visible site of temperature k, from the hidden states h."""
    W, b_v, b_a, h = f64(W, b_v, b_a, h)
    p = sigmoid((1.0 - beta) * b_a + beta * (h @ W.T + b_v))
    u = uniform(h.shape[0], W.shape[0], seed, STREAM_AIS_V, k, chain0)
    return p, u, (u < p).astype(np.float64)


def run(W, b_h, b_v, b_a, betas, n_chains, chain0, seed):
    """The whole run: (logw [n_chains], v_final, flagged [n_chains] -- some draw of the chain fell inside FLIP_BAND of its
    probability, so an fp32 evaluation may legitimately take the other branch there and part from this chain)."""
    betas = np.asarray(betas, dtype=np.float64)
    b_a64 = np.asarray(b_a, dtype=np.float64)
    p0 = np.broadcast_to(sigmoid(b_a64), (n_chains, b_a64.size))
    u0 = uniform(n_chains, b_a64.size, seed, STREAM_AIS_INIT, 0, chain0)
    v = (u0 < p0).astype(np.float64)
    flagged = (np.abs(u0 - p0) <= FLIP_BAND).any(axis=1)
    logw = np.zeros(n_chains)
    for k in range(1, betas.size):
        logw += delta(W, b_h, b_v, b_a, betas[k - 1], betas[k], v)[0]
        ph, uh, h = hidden(W, b_h, betas[k], k, v, chain0, seed)
        pv, uv, v = visible(W, b_v, b_a, betas[k], k, h, chain0, seed)
        flagged |= (np.abs(uh - ph) <= FLIP_BAND).any(axis=1) | (np.abs(uv - pv) <= FLIP_BAND).any(axis=1)
    return logw, v, flagged


def log_mean_exp(x):
    m = np.max(x)
    return float(m + np.log(np.mean(np.exp(x - m))))


def stderr(logw):
    """Delta-method standard error of log mean exp(logw): std(w) / (mean(w) sqrt(M)), w = exp(logw - max)."""
    w = np.exp(logw - np.max(logw))
    return float(np.std(w) / (np.mean(w) * np.sqrt(w.size)))


def log_z0(b_a, n_hid):
    return float(n_hid * np.log(2.0) + softplus(np.asarray(b_a, dtype=np.float64)).sum())


def brute_force_log_z(W, b_h, b_v):
    """log sum over ALL visible states of exp(-F(v)), written out: the check of ais.exact_log_partition."""
    W, b_h, b_v = f64(W, b_h, b_v)
    n = W.shape[0]
    assert n <= 16
    S = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)
    e = S @ b_v + softplus(S @ W + b_h).sum(axis=1)
    m = e.max()
    return float(m + np.log(np.exp(e - m).sum()))


# ---- the models of the free-run and estimate tests (shared by the GPU and the CPU tier; computed once per process) ----------
def normal_params(seed, n_vis, n_hid, w_std, b_std):
    """W, then b_h, b_v, b_A, in that order, from default_rng(seed); fp32 values."""
    g = np.random.default_rng(seed)
    W = g.normal(0.0, w_std, (n_vis, n_hid)).astype(np.float32)
    b_h = g.normal(0.0, b_std, n_hid).astype(np.float32)
    b_v = g.normal(0.0, b_std, n_vis).astype(np.float32)
    b_a = g.normal(0.0, b_std, n_vis).astype(np.float32)
    return W, b_h, b_v, b_a


FREE_BETAS = np.array([0, .1, .25, .4, .55, .7, .8, .9, 1], dtype=np.float64)
FREE_CHAINS, FREE_SHAPE = 200, (70, 36)
EST_CHAINS, EST_SHAPE, EST_TEMPS = 256, (13, 11), 500


def free_params(seed):
    return normal_params(200 + seed, FREE_SHAPE[0], FREE_SHAPE[1], 0.3, 0.3)


@functools.lru_cache(maxsize=None)
def free_run(seed):
    """Restatement of the short free run (200 chains, 70 x 36, nine temperatures) for `seed`."""
    return run(*free_params(seed), FREE_BETAS, FREE_CHAINS, 0, seed)


def est_params(seed):
    return normal_params(100 + seed, EST_SHAPE[0], EST_SHAPE[1], 0.6, 0.4)


@functools.lru_cache(maxsize=None)
def est_run(seed):
    """Restatement of the estimate test (13 x 11, 256 chains, 500 linear temperatures): (log Z estimate, SE, logw)."""
    W, b_h, b_v, b_a = est_params(seed)
    betas = np.arange(EST_TEMPS + 1, dtype=np.float64) / EST_TEMPS
    logw, _, _ = run(W, b_h, b_v, b_a, betas, EST_CHAINS, 0, seed)
    return log_z0(b_a, EST_SHAPE[1]) + log_mean_exp(logw), stderr(logw), logw
