"""Float64 restatement of the softmax label units of include/kurbm.h: the label site, the class logits and the CD step with
labels.  TEST INFRASTRUCTURE: the yardstick of tests/test_gpu_labels.py, itself checked on the CPU by tests/test_labels_host.py
(enumeration, draw frequencies, the margins of the fixtures).  Uniforms come from oracle.philox.uniform -- the fp32 values the
kernels compare against; everything else is float64.

A label RBM has n_vis = n_pix + C visible units; the last C columns are the label block.
"""
import math

import numpy as np

from oracle import philox

FLIP_BAND = 1e-5     # |u - p| (or |u - a cumulative boundary|) below which an fp32 draw may legitimately differ from this one
TOL_P = 1e-4         # the project's fp32 bar on probabilities
TOL_GEMM = 4e-6      # ... on sums of fp32 products, relative to the un-cancelled magnitude
TOL_STEP = 1e-4      # ... on a parameter update: |d - d_ref| <= TOL_STEP max(1, |d_ref|)   


def f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def one_hot(y, C):
    y = np.asarray(y, dtype=np.int64).reshape(-1)
    out = np.zeros((y.size, C), np.float32)
    out[np.arange(y.size), y] = 1.0
    return out


def stream_h(t, chain=0):
    return chain * 64 + 2 * t


def stream_v(t, chain=0):
    return chain * 64 + 2 * t - 1


# ---- the label site ---------------------------------------------------------------------------------------------------------
def label_probs(W, b_v, h, n_pix):
    """p = softmax(b_v[n_pix:] + h.W[n_pix:]^T), [rows, C]."""
    W, b_v, h = f64(W, b_v, h)
    x = h @ W[n_pix:].T + b_v[n_pix:]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def label_uniform(rows, n_pix, seed, stream_id, step, row0=0):
    """u(row, col = n_pix): ONE uniform per row, fp32."""
    return philox.uniform(rows, n_pix + 1, seed, stream_id, step, row0)[:, n_pix]


def draw_class(p, u):
    """First c with u < p_0 + .. + p_c, else C - 1.  Returns (classes, margin): margin[r] = the distance of u[r] to the nearest
    cumulative boundary (the last one, 1, is no boundary: u < 1 always)."""
    cum = np.cumsum(p, axis=1)
    below = u[:, None].astype(np.float64) < cum
    cls = np.where(below.any(axis=1), below.argmax(axis=1), p.shape[1] - 1)
    margin = np.abs(u[:, None].astype(np.float64) - cum[:, :-1]).min(axis=1)
    return cls, margin


def label_site(W, b_v, h, n_pix, seed, stream_id, step, row0=0):
    """(p [rows, C], u [rows] fp32, classes [rows], margin [rows]) of the label site for the hidden states h."""
    p = label_probs(W, b_v, h, n_pix)
    u = label_uniform(p.shape[0], n_pix, seed, stream_id, step, row0)
    cls, margin = draw_class(p, u)
    return p, u, cls, margin


# ---- class logits -----------------------------------------------------------------------------------------------------------
def class_logits(W, b_h, b_v, v_pix, n_pix):
    """(logits [rows, C], abs_terms [rows, C]): logit_c = b_v[n_pix + c] + sum_j softplus(a_j + W[n_pix + c, j]), a = v.W[:n_pix] +
    b_h; abs_terms = |b_v| + the same sum (softplus >= 0), the un-cancelled magnitude a tolerance is relative to."""
    W, b_h, b_v, v = f64(W, b_h, b_v, v_pix)
    a = v[:, :n_pix] @ W[:n_pix] + b_h                               # [rows, n_hid]
    sp = softplus(a[:, None, :] + W[n_pix:][None, :, :]).sum(axis=2)    # [rows, C]
    return sp + b_v[n_pix:], sp + np.abs(b_v[n_pix:])


def posterior(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def joint_free_energy(W, b_h, b_v, v_pix, n_pix):
    """F(v, y = c) = -v.b_v[:n_pix] - logit_c, [rows, C]."""
    logits, _ = class_logits(W, b_h, b_v, v_pix, n_pix)
    v, bv = f64(v_pix, b_v)
    return -(v[:, :n_pix] @ bv[:n_pix])[:, None] - logits


def exact_posterior(W, b_h, b_v, v_pix, n_pix):
    """p(y | v) by brute force: the joint exp(-E(v, y, h)) summed over every hidden state, one class at a time."""
    W, b_h, b_v, v = f64(W, b_h, b_v, v_pix)
    n_hid, C = W.shape[1], W.shape[0] - n_pix
    H = ((np.arange(1 << n_hid)[:, None] >> np.arange(n_hid)[None, :]) & 1).astype(np.float64)
    out = np.zeros((v.shape[0], C))
    for r in range(v.shape[0]):
        for c in range(C):
            full = np.concatenate([v[r, :n_pix], np.eye(C)[c]])
            out[r, c] = np.exp(full @ b_v + H @ b_h + H @ (full @ W)).sum()
    return out / out.sum(axis=1, keepdims=True)


# ---- the CD step with labels ------------------------------------------------------------------------------------------------
def cd_step(W, b_h, b_v, v_batch, n_labels, seed, step, k=1, row0=0, chain=0, v_chain=None):
    """One CD-k chain with the label site behind every h -> v half step, from float64 copies of the fp32 parameters.
    Returns a dict: dW, db_h, db_v (batch sums), v_neg, h_pos, h_neg, and `margin`, the smallest |u - p| of every Bernoulli draw
    and |u - boundary| of every label draw of the chain."""
    W, b_h, b_v, v_pos = f64(W, b_h, b_v, v_batch)
    n_pix = W.shape[0] - n_labels
    rows, n_vis, n_hid = v_pos.shape[0], W.shape[0], W.shape[1]
    margin = [np.inf]

    def bern(p, stream_id):
        u = philox.uniform(p.shape[0], p.shape[1], seed, stream_id, step, row0)
        margin[0] = min(margin[0], float(np.abs(u.astype(np.float64) - p).min()))
        return (u.astype(np.float64) < p).astype(np.float64)

    h_pos = bern(sigmoid(v_pos @ W + b_h), stream_h(0, chain))
    h = h_pos if v_chain is None else bern(sigmoid(f64(v_chain)[0] @ W + b_h), stream_h(0, chain) + 32)
    v = None
    for t in range(1, k + 1):
        p_v = sigmoid(h @ W.T + b_v)
        # (the Bernoulli draws of the label columns are overwritten: their margins do not count)
        u = philox.uniform(rows, n_vis, seed, stream_v(t, chain), step, row0).astype(np.float64)
        margin[0] = min(margin[0], float(np.abs(u[:, :n_pix] - p_v[:, :n_pix]).min()))
        v = (u < p_v).astype(np.float64)
        _, _, cls, m = label_site(W, b_v, h, n_pix, seed, stream_v(t, chain), step, row0)
        margin[0] = min(margin[0], float(m.min()))
        v[:, n_pix:] = one_hot(cls, n_labels)
        if t < k:
            h = bern(sigmoid(v @ W + b_h), stream_h(t, chain))
    h_neg = sigmoid(v @ W + b_h)
    return {"dW": v_pos.T @ h_pos - v.T @ h_neg, "db_h": h_pos.sum(axis=0) - h_neg.sum(axis=0), "db_v": v_pos.sum(axis=0) - v.sum(axis=0),
            "abs_dW": v_pos.T @ h_pos + v.T @ h_neg, "abs_db_h": h_pos.sum(axis=0) + h_neg.sum(axis=0),
            "v_neg": v, "h_pos": h_pos, "h_neg": h_neg, "margin": margin[0]}


def fit(W, b_h, b_v, V, n_labels, batch_size, epochs, lr, seed, step0=0):
    """RBM.fit(verbose = 0) of a label RBM: contiguous batches, remainder last, one fused CD-1 update each, parameters kept in
    float64 between the steps.  Returns (W, b_h, b_v, next step, smallest margin of any draw)."""
    W, b_h, b_v = [x.copy() for x in f64(W, b_h, b_v)]
    step, margin = step0, np.inf
    for _ in range(epochs):
        for lo in range(0, V.shape[0], batch_size):
            s = cd_step(W, b_h, b_v, V[lo:lo + batch_size], n_labels, seed, step)
            W, b_h, b_v = W + lr * s["dW"], b_h + lr * s["db_h"], b_v + lr * s["db_v"]
            margin = min(margin, s["margin"])
            step += 1
    return W, b_h, b_v, step, margin


def predict(W, b_h, b_v, v_pix, n_pix):
    return class_logits(W, b_h, b_v, v_pix, n_pix)[0].argmax(axis=1)


# ---- fixtures shared by the CPU and the GPU tier -------------------------------------------------------------------------
SITE_SHAPES = [(200, 37, 10, 52), (200, 37, 3, 52), (133, 64, 10, 96), (70, 20, 64, 36)]     # (rows, n_pix, C, n_hid)
SITE_SEED, SITE_STREAM, SITE_STEP = 42, 1, 7
# k_label_sample walks the hidden units in blocks of 64, two blocks per turn of its main loop (one register set each), then a
# guarded tail of n_hid % 64 units; up to 16 classes are one block of classes, more are four.  The shapes above have n_hid <= 96:
# the tail alone, or one block and a tail.  These reach the loop: (full blocks, tail) = (3, 8), (4, 4), (2, 0), (3, 0), the first
# and third with one block of classes, the others with four.  Same inputs, seeds and site as the shapes above.
LOOP_SHAPES = [(70, 20, 10, 200), (70, 20, 40, 260), (40, 20, 10, 128), (40, 20, 40, 192)]


def site_inputs(rows, n_pix, C, n_hid):
    g = np.random.default_rng(31)
    W = g.normal(0, .3, (n_pix + C, n_hid)).astype(np.float32)
    b_v = g.normal(0, .3, n_pix + C).astype(np.float32)
    h = (np.random.default_rng(3).random((rows, n_hid)) < .5).astype(np.float32)
    return W, b_v, h


def model(n_pix, C, n_hid, seed=31, std=.3):
    g = np.random.default_rng(seed)
    W = g.normal(0, std, (n_pix + C, n_hid)).astype(np.float32)
    b_h = g.normal(0, std, n_hid).astype(np.float32)
    b_v = g.normal(0, std, n_pix + C).astype(np.float32)
    return W, b_h, b_v


def labelled_batch(rows, n_pix, C, seed=5):
    """[pixels | one-hot label] fp32 [rows, n_pix + C] and the labels."""
    g = np.random.default_rng(seed)
    pix = (g.random((rows, n_pix)) < .5).astype(np.float32)
    y = g.integers(0, C, rows)
    return np.concatenate([pix, one_hot(y, C)], axis=1), y


ANCHOR = (64, 37, 10, 52)        # the anchored step: (rows, n_pix, C, n_hid), seed / step below
ANCHOR_SEED, ANCHOR_STEP = 42, 3
FIT_SHAPE = (150, 37, 10, 52)    # the host trajectory: N = 150, batch 64 -> two full batches and a remainder of 22
FIT_BATCH, FIT_LR, FIT_SEED = 64, 1e-3, 42


def prototypes_data(n_rows=512, n_pix=32, C=4, flip=0.05, seed=17):
    """C prototype classes of n_pix pixels, each pixel flipped with probability `flip`."""
    g = np.random.default_rng(seed)
    protos = (g.random((C, n_pix)) < .5).astype(np.float32)
    y = g.integers(0, C, n_rows)
    flips = g.random((n_rows, n_pix)) < flip
    return np.abs(protos[y] - flips.astype(np.float32)), y


LEARN = dict(n_pix=32, C=4, n_hid=32, batch=64, epochs=10, lr=0.01, seed=7)


def learn_init():
    g = np.random.default_rng(LEARN["seed"])
    nv, nh = LEARN["n_pix"] + LEARN["C"], LEARN["n_hid"]
    return (g.uniform(-0.05, 0.05, (nv, nh)).astype(np.float32), g.uniform(-0.05, 0.05, nh).astype(np.float32),
            g.uniform(-0.05, 0.05, nv).astype(np.float32))


# ---- chi-square survival function (no scipy in the test tier) ----------------------------------------------------------------
def chi2_sf(x, dof):
    """P(chi^2_dof > x) = Q(dof / 2, x / 2), the regularised upper incomplete gamma function: its series below a + 1, the
    continued fraction (modified Lentz) above."""
    a, x = dof / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-15:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-15:
            break
    return math.exp(-x + a * math.log(x) - lg) * h
