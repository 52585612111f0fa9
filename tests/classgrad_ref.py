"""Float64 restatement of the discriminative gradient of a label RBM (include/kurbm.h, "discriminative and hybrid training").
TEST INFRASTRUCTURE: the yardstick of tests/test_gpu_classgrad.py, itself checked on the CPU by tests/test_classgrad_host.py
(central differences of sum log p(y | v), the learning run).  The same formulas in numpy float32 (class_grad_fp32) give the
rounding noise an fp32 evaluation has at a fixture's shape: the GPU tier's bars are multiples of it.

Notation of the header: n_vis = n_pix + C, U = W[n_pix:], d = b_v[n_pix:], a = v_pix.W[:n_pix] + b_h, o_cj = a_j + U_cj,
logit_c = d_c + sum_j softplus(o_cj), p = softmax(logit), t the one-hot block, q = t - p.
"""
import numpy as np

import labels_ref as R


def _grad(W, b_h, b_v, v_batch, n_labels, dt):
    W, b_h, b_v, v = [np.asarray(x, dtype=dt) for x in (W, b_h, b_v, v_batch)]
    C = int(n_labels)
    n_pix = W.shape[0] - C
    rows = v.shape[0]
    one = dt(1.0)
    v_pix, t = v[:, :n_pix], v[:, n_pix:]
    y = t.argmax(axis=1)
    a = v_pix @ W[:n_pix] + b_h                                   # [rows, n_hid]
    o = a[:, None, :] + W[n_pix:][None, :, :]                     # [rows, C, n_hid]
    sp = np.maximum(o, dt(0)) + np.log1p(np.exp(-np.abs(o)))
    logit = sp.sum(axis=2) + b_v[n_pix:]
    m = logit.max(axis=1, keepdims=True)
    e = np.exp(logit - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    nll = (m[:, 0] - logit[np.arange(rows), y]) + np.log(s[:, 0])
    with np.errstate(over="ignore"):
        sig = one / (one + np.exp(-o))                            # (exp overflows to inf for a very negative o: 1 / inf = 0, as wanted)
    q = t - p
    S_y = sig[np.arange(rows), y, :]
    H_bar = (p[:, :, None] * sig).sum(axis=1)
    g = S_y - H_bar
    dW = np.concatenate([v_pix.T @ S_y - v_pix.T @ H_bar, (q[:, :, None] * sig).sum(axis=0)], axis=0)
    abs_dW = np.concatenate([np.abs(v_pix).T @ (S_y + H_bar), ((t + p)[:, :, None] * sig).sum(axis=0)], axis=0)
    db_v = np.concatenate([np.zeros(n_pix, dt), q.sum(axis=0)])
    abs_db_v = np.concatenate([np.zeros(n_pix, dt), (t + p).sum(axis=0)])
    return {"S_y": S_y, "H_bar": H_bar, "g": g, "nll": nll, "p": p, "logits": logit, "y": y,
            "dW": dW, "db_h": g.sum(axis=0), "db_v": db_v,
            "abs_dW": abs_dW, "abs_db_h": (S_y + H_bar).sum(axis=0), "abs_db_v": abs_db_v}


def class_grad(W, b_h, b_v, v_batch, n_labels):
    """The gradient of sum_rows log p(y | v) and its operands, float64, for v_batch [rows, n_pix + C] (label block last): S_y,
    H_bar, g [rows, n_hid], nll [rows], dW [n_vis, n_hid], db_h, db_v (batch SUMS) and the un-cancelled magnitudes abs_dW
    (|v|^T (S_y + H_bar) for pixel rows, sum (t + p) sigma for label rows), abs_db_h, abs_db_v a tolerance is relative to."""
    return _grad(W, b_h, b_v, v_batch, n_labels, np.float64)


def class_grad_fp32(W, b_h, b_v, v_batch, n_labels):
    """The same formulas evaluated in numpy float32: what fp32 rounding alone does to them at this shape."""
    return _grad(W, b_h, b_v, v_batch, n_labels, np.float32)


def packed(out, prefix=""):
    """[dW | db_h | db_v] of a class_grad dict as one vector (prefix 'abs_' for the magnitudes)."""
    return np.concatenate([out[prefix + "dW"].reshape(-1), out[prefix + "db_h"], out[prefix + "db_v"]])


def mean_log_posterior(W, b_h, b_v, V, n_labels):
    """mean_rows log p(y | v), float64."""
    return float(-class_grad(W, b_h, b_v, V, n_labels)["nll"].mean())


def disc_fit(W, b_h, b_v, V, n_labels, batch_size, epochs, lr):
    """RBM.fit(verbose = 0, objective = 'discriminative'): contiguous batches, remainder last, params += lr * the batch sums,
    parameters kept in float64 between the steps.  Returns (W, b_h, b_v, number of steps)."""
    W, b_h, b_v = [x.copy() for x in R.f64(W, b_h, b_v)]
    steps = 0
    for _ in range(epochs):
        for lo in range(0, V.shape[0], batch_size):
            s = class_grad(W, b_h, b_v, V[lo:lo + batch_size], n_labels)
            W, b_h, b_v = W + lr * s["dW"], b_h + lr * s["db_h"], b_v + lr * s["db_v"]
            steps += 1
    return W, b_h, b_v, steps


def hybrid_step(W, b_h, b_v, v_batch, n_labels, gen_weight, seed, step, k=1, chain=0, v_chain=None):
    """The packed sums of one hybrid update, delta_disc + gen_weight * delta_gen, both at the same parameters: class_grad and
    labels_ref.cd_step with the step's RNG coordinates.  Returns (dW, db_h, db_v, the generative step's dict)."""
    dsc = class_grad(W, b_h, b_v, v_batch, n_labels)
    gen = R.cd_step(W, b_h, b_v, v_batch, n_labels, seed, step, k=k, chain=chain, v_chain=v_chain)
    return (dsc["dW"] + gen_weight * gen["dW"], dsc["db_h"] + gen_weight * gen["db_h"], dsc["db_v"] + gen_weight * gen["db_v"], gen)
