"""Host side of the AIS log-partition estimate (Salakhutdinov & Murray 2008) for Bernoulli-Bernoulli RBMs: schedules, the
base-rate model, the estimate from the chains' log weights, and the exact log Z of models small enough to enumerate.

Everything here is numpy float64 and needs no device; the chains themselves run in libkurbm.so (kurbm_ais_run).
"""
import numpy as np


def beta_schedule(n, kind="linear"):
    """n + 1 inverse temperatures 0 = beta_0 < ... < beta_n = 1 (n annealing steps).

    'linear': equal spacing.  'three_stage': half of the steps on [0, 0.5], 40 % on [0.5, 0.9], the rest on [0.9, 1] --
    the spacing tightens towards the target, where the intermediate distributions change fastest (the paper's schedule)."""
    n = int(n)
    if n < 1:
        raise ValueError("a schedule needs at least one step, got %d" % n)
    if kind == "linear":
        b = np.arange(n + 1, dtype=np.float64) / n
    elif kind == "three_stage":
        if n < 3:
            raise ValueError("the three-stage schedule needs at least 3 steps, got %d" % n)
        n1 = max(1, min(n - 2, int(round(0.5 * n))))
        n2 = max(1, min(n - n1 - 1, int(round(0.4 * n))))
        n3 = n - n1 - n2
        b = np.concatenate([np.arange(n1, dtype=np.float64) / n1 * 0.5,
                            0.5 + np.arange(n2, dtype=np.float64) / n2 * 0.4,
                            0.9 + np.arange(n3 + 1, dtype=np.float64) / n3 * 0.1])
    else:
        raise ValueError("kind must be 'linear' or 'three_stage', got %r" % (kind,))
    b[0], b[-1] = 0.0, 1.0
    return b


def check_schedule(betas):
    """betas as a float64 vector, or ValueError unless it runs from 0 to 1 strictly increasing."""
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if b.size < 2 or b[0] != 0.0 or b[-1] != 1.0 or not np.all(np.diff(b) > 0):
        raise ValueError("betas must start at 0, end at 1 and be strictly increasing")
    return b


def base_rate_bias(V, smoothing=0.05, n_labels=0):
    """Visible bias b_A of the base-rate model (W = 0) of data V [rows, n_vis]: the logit of the column means, smoothed
    towards 1/2 -- p = (1 - smoothing) mean + smoothing / 2 -- so that an all-zero or all-one column stays finite.
    n_labels = C > 0: the last C columns are a one-hot label block, a softmax unit whose base model is categorical -- its
    entries are log((1 - smoothing) freq_c + smoothing / C), the log of the smoothed class frequencies."""
    if not 0.0 < smoothing <= 1.0:
        raise ValueError("smoothing must be in (0, 1]")
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[0] == 0:
        raise ValueError("expected a non-empty [rows, n_vis] matrix")
    n_labels = _check_labels(n_labels, V.shape[1])
    mean = np.clip(V.mean(axis=0), 0.0, 1.0)
    p = (1.0 - smoothing) * mean + 0.5 * smoothing
    b = np.log(p) - np.log1p(-p)
    if n_labels:
        b[-n_labels:] = np.log((1.0 - smoothing) * mean[-n_labels:] + smoothing / n_labels)
    return b


def _check_labels(n_labels, n_vis):
    n_labels = int(n_labels)
    if n_labels and not (2 <= n_labels <= 64 and n_labels < n_vis):
        raise ValueError("n_labels must be 0 or in [2, 64] and below n_vis = %d, got %d" % (n_vis, n_labels))
    return n_labels


def _logsumexp(x, axis=None):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    out = np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True)) + m
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def log_mean_exp(x):
    """log(mean(exp(x))) without overflow."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    m = np.max(x)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.mean(np.exp(x - m))))


def log_z0(base_bias, n_hid, n_labels=0):
    """log Z of the base-rate model: n_hid ln 2 + sum_i softplus(b_A,i); with a label block of n_labels = C units (the last
    C entries) n_hid ln 2 + sum_{i < n_pix} softplus(b_A,i) + logsumexp_c b_A[n_pix + c]."""
    b = np.asarray(base_bias, dtype=np.float64).reshape(-1)
    n_labels = _check_labels(n_labels, b.size)
    n_pix = b.size - n_labels
    z = n_hid * np.log(2.0) + np.sum(np.logaddexp(0.0, b[:n_pix]))
    if n_labels:
        z += _logsumexp(b[n_pix:])
    return float(z)


def estimate(logw, base_bias, n_hid, n_labels=0):
    """(log Z estimate, its standard error, log Z_0) from the chains' log weights.  The standard error is the delta method's:
    std(w) / (mean(w) sqrt(M)) on w = exp(logw - max).  n_labels: as log_z0."""
    logw = np.asarray(logw, dtype=np.float64).reshape(-1)
    z0 = log_z0(base_bias, n_hid, n_labels)
    w = np.exp(logw - np.max(logw))
    stderr = float(np.std(w) / (np.mean(w) * np.sqrt(w.size)))
    return z0 + log_mean_exp(logw), stderr, z0


def exact_log_partition(W, b_h, b_v, n_labels=0):
    """Exact log Z = log sum_v exp(-F(v)) by enumerating the states of the SMALLER layer (the other one sums in closed form).
    ValueError when min(n_vis, n_hid) > 24.
    n_labels = C > 0: the last C visible units are a one-hot label block, Z = sum over (pixels, class, h).  Enumerating the
    hidden side sums the block in closed form (logsumexp_c (b_v + W h)[n_pix + c] beside the pixels' softplus terms);
    enumerating the visible side runs over pixels x classes.  The smaller of n_hid and n_pix is enumerated."""
    W = np.asarray(W, dtype=np.float64)
    b_h = np.asarray(b_h, dtype=np.float64).reshape(-1)
    b_v = np.asarray(b_v, dtype=np.float64).reshape(-1)
    if W.shape != (b_v.size, b_h.size):
        raise ValueError("W has shape %s, expected %s" % (W.shape, (b_v.size, b_h.size)))
    n_labels = _check_labels(n_labels, b_v.size)
    if n_labels:
        return _exact_log_partition_labels(W, b_h, b_v, n_labels)
    if W.shape[1] < W.shape[0]:          # enumerate the hiddens: the same sum with the roles swapped
        W, b_h, b_v = W.T, b_v, b_h
    n = W.shape[0]
    if n > 24:
        raise ValueError("exact_log_partition enumerates 2^min(n_vis, n_hid) states: %d units is too many (at most 24)" % n)
    total = -np.inf
    for S in _states(n):
        e = S @ b_v + np.logaddexp(0.0, S @ W + b_h).sum(axis=1)
        total = np.logaddexp(total, _logsumexp(e))
    return float(total)


def _states(n):
    """Every 0/1 vector of n units, in blocks of 2^14 rows (float64)."""
    bits = np.arange(n, dtype=np.int64)
    for lo in range(0, 1 << n, 1 << 14):
        idx = np.arange(lo, min(lo + (1 << 14), 1 << n), dtype=np.int64)
        yield ((idx[:, None] >> bits[None, :]) & 1).astype(np.float64)


def _exact_log_partition_labels(W, b_h, b_v, C):
    n_pix, n_hid = b_v.size - C, b_h.size
    n = min(n_pix, n_hid)
    if n > 24:
        raise ValueError("exact_log_partition enumerates 2^min(n_pix, n_hid) states: %d units is too many (at most 24)" % n)
    total = -np.inf
    if n_hid <= n_pix:       # hidden states: pixels and the block sum in closed form
        for H in _states(n_hid):
            x = H @ W.T + b_v
            e = H @ b_h + np.logaddexp(0.0, x[:, :n_pix]).sum(axis=1) + _logsumexp(x[:, n_pix:], axis=1)
            total = np.logaddexp(total, _logsumexp(e))
    else:                    # pixel states x classes: the hiddens sum in closed form
        for S in _states(n_pix):
            a = S @ W[:n_pix] + b_h
            for c in range(C):
                e = S @ b_v[:n_pix] + b_v[n_pix + c] + np.logaddexp(0.0, a + W[n_pix + c]).sum(axis=1)
                total = np.logaddexp(total, _logsumexp(e))
    return float(total)


__all__ = ["beta_schedule", "check_schedule", "base_rate_bias", "log_mean_exp", "log_z0", "estimate", "exact_log_partition"]
