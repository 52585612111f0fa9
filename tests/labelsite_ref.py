"""Float64 restatement of the free label blocks of include/kurbm.h: the Gibbs sweep with the softmax site in it
(kurbm_gibbs_run_labels) and the AIS chain over [pixels | one-hot] (kurbm_ais_run_labels).  TEST INFRASTRUCTURE: the yardstick of
tests/test_gpu_labelsite.py, itself checked on the CPU by tests/test_labelsite_host.py (the enumerated joint distribution, label-
aware enumeration of log Z, the flag rates of every GPU fixture).  Uniforms come from oracle.philox; everything else is float64.

A label RBM has n_vis = n_pix + C visible units; the last C columns are the label block.
"""
import functools

import numpy as np

import ais_ref as A
import gibbs_ref as G
import labels_ref as L
from oracle import philox

FLIP_BAND = G.FLIP_BAND     # |u - p|, or |u - a cumulative boundary|, below which an fp32 draw may legitimately differ
TOL = G.TOL
FLAG_CAP = 0.10             # at most this share of a fixture's chains may be flagged (the issue's cap)


def softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def logsumexp(x, axis=None):
    m = np.max(x, axis=axis, keepdims=True)
    out = m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))
    return float(out.reshape(())) if axis is None else np.squeeze(out, axis=axis)


def draw_block(p, u):
    """(classes, near): the label site's draw for probabilities p [rows, C] and uniforms u [rows]; near[r]: u[r] lies within
    FLIP_BAND of a cumulative boundary."""
    cls, margin = L.draw_class(p, np.asarray(u))
    return cls, margin <= FLIP_BAND


# ---- Gibbs with a free block ------------------------------------------------------------------------------------------------
def gibbs_run(W, b_h, b_v, v_init, n_labels, chain0, seed, burn_in=1, thin=1, n_keep=1, clamp=None):
    """The run of kurbm_gibbs_run_labels: (v_kept [n_keep, n_chains, n_vis], prob_kept likewise -- block columns: the softmax p --,
    flagged [n_chains]).  A chain is flagged when a Bernoulli draw (hidden, or a PIXEL) lies within FLIP_BAND of its probability, or
    its label uniform within FLIP_BAND of a cumulative boundary.  The label entries of clamp are ignored: the block is free."""
    W64, bh64, bv64 = G.f64(W, b_h, b_v)
    v0 = np.asarray(v_init, dtype=np.float64)
    n, nv = v0.shape
    C = int(n_labels)
    n_pix = nv - C
    m = G.mask_of(clamp, nv)
    m[n_pix:] = False
    T = burn_in + (n_keep - 1) * thin
    v = v0.copy()
    flagged = np.zeros(n, dtype=bool)
    vs, ps = [], []
    for t in range(1, T + 1):
        ph = G.sigmoid(v @ W64 + bh64)
        uh = G.uniform(n, W64.shape[1], seed, G.STREAM_GIBBS_H, t, chain0)
        h = (uh < ph).astype(np.float64)
        flagged |= (np.abs(uh - ph) <= FLIP_BAND).any(axis=1)
        x = h @ W64.T + bv64
        pv = G.sigmoid(x)
        uv = philox.uniform(n, nv, seed, G.STREAM_GIBBS_V, t, row0=chain0)       # fp32: column n_pix is the label uniform
        uv64 = uv.astype(np.float64)
        v = (uv64 < pv).astype(np.float64)
        flagged |= (np.abs(uv64[:, :n_pix] - pv[:, :n_pix]) <= FLIP_BAND).any(axis=1)
        py = softmax(x[:, n_pix:])
        cls, near = draw_block(py, uv[:, n_pix])
        flagged |= near
        v[:, n_pix:] = L.one_hot(cls, C)
        pv = pv.copy()
        pv[:, n_pix:] = py
        v[:, m] = v0[:, m]
        if t >= burn_in and (t - burn_in) % thin == 0:
            pv[:, m] = v0[:, m]
            vs.append(v.copy())
            ps.append(pv)
    return np.stack(vs), np.stack(ps), flagged


def start_block(b_v, n_pix, n_chains, chain0, seed):
    """The classes RBM.sample(label='free', init=None) starts from: softmax(b_v[n_pix:]) with u(row, n_pix) at (GIBBS_V, 0)."""
    p = softmax(np.asarray(b_v, dtype=np.float64)[None, n_pix:])
    u = L.label_uniform(n_chains, n_pix, seed, G.STREAM_GIBBS_V, 0, chain0)
    return draw_block(np.repeat(p, n_chains, axis=0), u)[0]


# ---- the enumerated joint distribution of a small label RBM -----------------------------------------------------------------
def joint_states(n_pix, C):
    """All 2^n_pix * C states [pixels | one-hot]; index = pixel index + 2^n_pix * class."""
    S = G.state_matrix(n_pix)
    return np.concatenate([np.concatenate([S, np.repeat(L.one_hot([c], C), S.shape[0], axis=0)], axis=1) for c in range(C)], axis=0)


def joint_index(v, n_pix):
    v = np.asarray(v)
    return G.state_index(v[:, :n_pix]) + (1 << n_pix) * v[:, n_pix:].argmax(axis=1)


def joint_log_pstar(W, b_h, b_v, S):
    W, b_h, b_v, S = G.f64(W, b_h, b_v, S)
    return S @ b_v + np.logaddexp(0.0, S @ W + b_h).sum(axis=1)


def exact_joint(W, b_h, b_v, n_pix, clamp=None, values=None):
    """p(v, y) over joint_states (with clamp / values on PIXELS: the conditional, zero elsewhere)."""
    C = np.asarray(W).shape[0] - n_pix
    S = joint_states(n_pix, C)
    e = joint_log_pstar(W, b_h, b_v, S)
    if clamp is not None:
        ok = (S[:, np.asarray(clamp)] == np.asarray(values, dtype=np.float64)[None, :]).all(axis=1)
        e = np.where(ok, e, -np.inf)
    p = np.exp(e - e.max())
    return p / p.sum()


def joint_band_violations(samples, p, n_pix, sigmas):
    """gibbs_ref.band_violations on the joint index."""
    N = samples.shape[0]
    f = np.bincount(joint_index(samples, n_pix), minlength=p.size) / float(N)
    bad = np.abs(f - p) > sigmas * np.sqrt(p * (1.0 - p) / N) + 1.0 / N
    return np.nonzero(bad)[0], f


def brute_force_log_z(W, b_h, b_v, n_pix):
    """log sum over EVERY (v, y, h) of exp(-E), written out: the check of ais.exact_log_partition(n_labels=C)."""
    W, b_h, b_v = G.f64(W, b_h, b_v)
    C, n_hid = W.shape[0] - n_pix, W.shape[1]
    assert n_pix + n_hid <= 20
    S = joint_states(n_pix, C)
    H = G.state_matrix(n_hid)
    total = -np.inf
    for s in S:
        e = s @ b_v + H @ b_h + H @ (s @ W)
        total = np.logaddexp(total, logsumexp(e))
    return float(total)


def log_joint(W, b_h, b_v, V_joined, log_z):
    """log p(v, y) per row of [pixels | one-hot]."""
    return joint_log_pstar(W, b_h, b_v, V_joined) - log_z


def log_marginal(W, b_h, b_v, v_pix, n_pix, log_z):
    """log p(v) = v.b_v[:n_pix] + logsumexp_c logit_c(v) - log Z per row."""
    logits, _ = L.class_logits(W, b_h, b_v, v_pix, n_pix)
    v, bv = G.f64(v_pix, b_v)
    return v[:, :n_pix] @ bv[:n_pix] + logsumexp(logits, axis=1) - log_z


# ---- AIS with a label block -------------------------------------------------------------------------------------------------
def ais_log_z0(b_a, n_hid, n_pix):
    b = np.asarray(b_a, dtype=np.float64)
    return float(n_hid * np.log(2.0) + A.softplus(b[:n_pix]).sum() + logsumexp(b[n_pix:]))


def ais_delta(W, b_h, b_v, b_a, beta_prev, beta, v):
    """(Delta_k, un-cancelled magnitude) per chain -- ais_ref.delta: on a one-hot block (b_v - b_A).v IS the pixel sum plus the
    term of the class that is on."""
    return A.delta(W, b_h, b_v, b_a, beta_prev, beta, v)


def ais_visible(W, b_v, b_a, beta, k, h, n_pix, chain0, seed):
    """The visible site of temperature k: (p_pix [rows, n_pix], u [rows, n_vis] fp32, p_y [rows, C], v [rows, n_vis], near [rows])."""
    W64, bv64, ba64, h64 = A.f64(W, b_v, b_a, h)
    x = (1.0 - beta) * ba64 + beta * (h64 @ W64.T + bv64)
    u = philox.uniform(h64.shape[0], W64.shape[0], seed, A.STREAM_AIS_V, k, row0=chain0)
    p = A.sigmoid(x[:, :n_pix])
    v = np.zeros_like(x)
    v[:, :n_pix] = u[:, :n_pix].astype(np.float64) < p
    py = softmax(x[:, n_pix:])
    cls, near = draw_block(py, u[:, n_pix])
    v[:, n_pix:] = L.one_hot(cls, py.shape[1])
    near = near | (np.abs(u[:, :n_pix].astype(np.float64) - p) <= FLIP_BAND).any(axis=1)
    return p, u, py, v, near


def ais_start(b_a, n_pix, n_chains, chain0, seed):
    ba = np.asarray(b_a, dtype=np.float64)
    u = philox.uniform(n_chains, ba.size, seed, A.STREAM_AIS_INIT, 0, row0=chain0)
    p = np.broadcast_to(A.sigmoid(ba[:n_pix]), (n_chains, n_pix))
    v = np.zeros((n_chains, ba.size))
    v[:, :n_pix] = u[:, :n_pix].astype(np.float64) < p
    py = np.repeat(softmax(ba[None, n_pix:]), n_chains, axis=0)
    cls, near = draw_block(py, u[:, n_pix])
    v[:, n_pix:] = L.one_hot(cls, ba.size - n_pix)
    return v, near | (np.abs(u[:, :n_pix].astype(np.float64) - p) <= FLIP_BAND).any(axis=1)


def ais_run(W, b_h, b_v, b_a, n_labels, betas, n_chains, chain0, seed):
    """(logw [n_chains], v_final, flagged)."""
    betas = np.asarray(betas, dtype=np.float64)
    n_pix = np.asarray(W).shape[0] - n_labels
    v, flagged = ais_start(b_a, n_pix, n_chains, chain0, seed)
    logw = np.zeros(n_chains)
    for k in range(1, betas.size):
        logw += ais_delta(W, b_h, b_v, b_a, betas[k - 1], betas[k], v)[0]
        ph, uh, h = A.hidden(W, b_h, betas[k], k, v, chain0, seed)
        _, _, _, v, near = ais_visible(W, b_v, b_a, betas[k], k, h, n_pix, chain0, seed)
        flagged = flagged | near | (np.abs(uh - ph) <= FLIP_BAND).any(axis=1)
    return logw, v, flagged


# ---- fixtures (shared by the GPU and the CPU tier; computed once per process) -----------------------------------------------
# (rows, n_pix, C, n_hid): the block straddles the 64-group of the permuted plane, n_hid < 64 | unaligned inside a group, n_hid
# tail past 3 x 64 | straddles the 128 padding boundary | the C > 16 path
GIBBS_SHAPES = [(37, 60, 10, 36), (200, 37, 3, 200), (130, 120, 10, 96), (70, 20, 64, 36)]
GIBBS_SEED = 3
KEEP = dict(burn_in=2, thin=3, n_keep=3)          # 8 sweeps
AIS_SHAPES = [(37, 60, 10, 36), (130, 290, 10, 200)]
AIS_BETAS = [(0.0, 0.1), (0.3, 0.4), (0.9, 1.0)]
AIS_SEED, AIS_K = 7, 5
RUN_BETAS = np.array([0, .2, .5, .8, 1], dtype=np.float64)
DIST = (6, 3, 5)                                  # the 192-state model of tests/test_labels_host.py: L.model(6, 3, 5)
DIST_CHAINS, DIST_BURN, DIST_SEED = 8192, 100, 5
DIST_CLAMP, DIST_VALUES = np.array([0, 3]), np.array([1.0, 0.0])
EST = (10, 3, 9)                                  # the AIS estimate: 10 pixels, 3 classes, 9 hidden units
EST_CHAINS, EST_TEMPS, EST_SEED = 256, 400, 2


def gibbs_model(shape):
    rows, n_pix, C, n_hid = shape
    return L.model(n_pix, C, n_hid, seed=600 + n_pix + C, std=.3)


def gibbs_init(shape, real=False):
    """[pixels | one-hot]; real: pixel values in [0, 1) that are no bf16 values (the clamped ones travel as three pieces)."""
    rows, n_pix, C, n_hid = shape
    g = np.random.default_rng(700 + n_pix + C)
    pix = g.random((rows, n_pix))
    pix = pix.astype(np.float32) if real else (pix < .5).astype(np.float32)
    return np.concatenate([pix, L.one_hot(g.integers(0, C, rows), C)], axis=1)


def gibbs_clamp(shape):
    """Pixels on both sides of the block's 8-byte group (and the first pixel): the clamp launch rewrites groups the block is in."""
    rows, n_pix, C, n_hid = shape
    return np.unique(np.array([0, max(n_pix - 9, 0), n_pix - 2, n_pix - 1]))


@functools.lru_cache(maxsize=None)
def gibbs_fixture(i, kind, chain0=0):
    """kind: 'free' (one kept sample after 8 sweeps), 'keep' (KEEP), 'clamp' (0/1 start, pixels clamped, KEEP), 'real' (real-valued
    start, pixels clamped, KEEP).  Returns (params, v_init, clamp, run kwargs, restated (v, prob, flagged))."""
    shape = GIBBS_SHAPES[i]
    W, b_h, b_v = gibbs_model(shape)
    v0 = gibbs_init(shape, real=kind == "real")
    clamp = gibbs_clamp(shape) if kind in ("clamp", "real") else None
    kw = dict(burn_in=8, thin=1, n_keep=1) if kind == "free" else dict(KEEP)
    ref = gibbs_run(W, b_h, b_v, v0, shape[2], chain0, GIBBS_SEED, clamp=clamp, **kw)
    return (W, b_h, b_v), v0, clamp, kw, ref


def ais_model(shape):
    rows, n_pix, C, n_hid = shape
    W, b_h, b_v = L.model(n_pix, C, n_hid, seed=800 + n_pix, std=.3)
    b_a = np.random.default_rng(810 + n_pix).normal(0, .3, n_pix + C).astype(np.float32)
    v = gibbs_init(shape)
    return W, b_h, b_v, b_a, v


def dist_model():
    return L.model(*DIST)


@functools.lru_cache(maxsize=None)
def dist_run(clamped):
    """The restatement's chains on the 192-state model: 8192 chains, 100 sweeps, one kept sample."""
    W, b_h, b_v = dist_model()
    n_pix, C, _ = DIST
    g = np.random.default_rng(79)
    v0 = np.concatenate([(g.random((DIST_CHAINS, n_pix)) < .5).astype(np.float32), L.one_hot(g.integers(0, C, DIST_CHAINS), C)], axis=1)
    if clamped:
        v0[:, DIST_CLAMP] = DIST_VALUES.astype(np.float32)[None, :]
    v, _, _ = gibbs_run(W, b_h, b_v, v0, C, 0, DIST_SEED, burn_in=DIST_BURN, clamp=DIST_CLAMP if clamped else None)
    return v0, v[0]


def est_model():
    n_pix, C, n_hid = EST
    W, b_h, b_v = L.model(n_pix, C, n_hid, seed=900, std=.6)
    b_a = np.random.default_rng(901).normal(0, .4, n_pix + C).astype(np.float32)
    return W, b_h, b_v, b_a


@functools.lru_cache(maxsize=None)
def est_run():
    """(log Z estimate, SE, logw) of the restatement on the enumerable model."""
    W, b_h, b_v, b_a = est_model()
    betas = np.arange(EST_TEMPS + 1, dtype=np.float64) / EST_TEMPS
    logw, _, _ = ais_run(W, b_h, b_v, b_a, EST[1], betas, EST_CHAINS, 0, EST_SEED)
    return ais_log_z0(b_a, EST[2], EST[0]) + A.log_mean_exp(logw), A.stderr(logw), logw
