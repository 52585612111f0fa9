"""Float64 restatement of fine-tuning a DBN on sum log p(y | v) by backpropagation (include/kurbm.h, "fine-tuning a DBN").
TEST INFRASTRUCTURE: the yardstick of tests/test_gpu_backprop.py, itself checked on the CPU by tests/test_backprop_host.py (central
differences of the loss, torch.autograd in float64, a learning run).  The same formulas in numpy float32 (dt=np.float32) give the
rounding noise an fp32 evaluation has at a fixture's shape: the GPU tier's bars are multiples of it.

The stack: `lower`, a list of (W [n_in, n_out], b_h, act) with act one of ACT_SIGMOID / ACT_RELU / ACT_LINEAR, under the label RBM
`top` = (W [n_pix + C, n_hid], b_h, b_v).  x_0 = V, x_l = act_l(x_{l-1}.W_l + b_h,l), the top layer sees [x_{L-1} | one-hot(y)]; going
down, delta_l = e_l * act_l'(x_l), dW_l = x_{l-1}^T.delta_l, db_h,l = sum_rows delta_l, e_{l-1} = delta_l.W_l^T.  Batch SUMS.
"""
import numpy as np

import classgrad_ref as G
import labels_ref as R

ACT_SIGMOID, ACT_RELU, ACT_LINEAR = 0, 1, 2        # KURBM_ACT_*


def activate(pre, act):
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-pre))
    if act == ACT_RELU:
        return np.maximum(pre, 0.0)
    if act == ACT_LINEAR:
        return pre
    raise ValueError(act)


def site(e, x_out, act):
    """delta = e * act'(x_out), the derivative written in the layer's OUTPUT: sigmoid x (1 - x), relu [x > 0], linear 1."""
    if act == ACT_SIGMOID:
        return e * (x_out * (1 - x_out))
    if act == ACT_RELU:
        return np.where(x_out > 0, e, np.zeros_like(e))
    if act == ACT_LINEAR:
        return e.copy()
    raise ValueError(act)


def forward(lower, V, dt=np.float64):
    """(xs, pres): xs[0] = V, xs[l] = act_l(pres[l - 1]), pres[l - 1] = xs[l - 1].W_l + b_h,l."""
    xs, pres = [np.asarray(V, dtype=dt)], []
    for W, b_h, act in lower:
        pres.append(xs[-1] @ np.asarray(W, dtype=dt) + np.asarray(b_h, dtype=dt))
        xs.append(activate(pres[-1], act))
    return xs, pres


def layer_backward(W, act, x_in, x_out, e, dt=np.float64, want_e_in=True):
    """One layer's share, from the planes it is GIVEN (x_out as the forward pass left it): delta, dW, db_h, e_in and the un-cancelled
    magnitudes abs_dW = |x_in|^T.|delta|, abs_db_h = sum |delta|, abs_e_in = |delta|.|W|^T a tolerance is relative to."""
    W, x_in, x_out, e = [np.asarray(a, dtype=dt) for a in (W, x_in, x_out, e)]
    delta = site(e, x_out, act)
    out = {"delta": delta, "dW": x_in.T @ delta, "db_h": delta.sum(axis=0), "db_v": np.zeros(W.shape[0], dt),
           "abs_dW": np.abs(x_in).T @ np.abs(delta), "abs_db_h": np.abs(delta).sum(axis=0)}
    if want_e_in:
        out["e_in"], out["abs_e_in"] = delta @ W.T, np.abs(delta) @ np.abs(W).T
    return out


def top_backward(top, C, v_top, dt=np.float64):
    """The top label RBM's share: classgrad_ref's dict (g, nll, dW, db_h, db_v and their magnitudes) with e_in = g.W[:n_pix]^T
    (no bias term) and abs_e_in = (S_y + H_bar).|W[:n_pix]|^T."""
    W, b_h, b_v = top
    out = dict(G._grad(W, b_h, b_v, v_top, C, dt))
    Wp = np.asarray(W, dtype=dt)[:W.shape[0] - C]
    out["e_in"], out["abs_e_in"] = out["g"] @ Wp.T, (out["S_y"] + out["H_bar"]) @ np.abs(Wp).T
    return out


def grad(lower, top, C, V, y, dt=np.float64):
    """The gradient of sum_rows log p(y | v) for every parameter block of the stack.  A dict: xs, pres (forward), top (top_backward's
    dict), layers (layer_backward's dict per lower layer, in stack order), nll [rows]."""
    xs, pres = forward(lower, V, dt)
    v_top = np.concatenate([xs[-1], R.one_hot(y, C).astype(dt)], axis=1)
    t = top_backward(top, C, v_top, dt)
    layers, e = [None] * len(lower), t["e_in"]
    for l in range(len(lower) - 1, -1, -1):
        layers[l] = layer_backward(lower[l][0], lower[l][2], xs[l], xs[l + 1], e, dt, want_e_in=l > 0)
        e = layers[l].get("e_in")
    return {"xs": xs, "pres": pres, "top": t, "layers": layers, "nll": t["nll"]}


def total_log_posterior(lower, top, C, V, y):
    """sum_rows log p(y | v), float64: the function `grad` differentiates."""
    xs, _ = forward(lower, V)
    W, b_h, b_v = top
    v_top = np.concatenate([xs[-1], R.one_hot(y, C).astype(np.float64)], axis=1)
    return float(-G.class_grad(W, b_h, b_v, v_top, C)["nll"].sum())


def mean_log_posterior(lower, top, C, V, y):
    return total_log_posterior(lower, top, C, V, y) / V.shape[0]


def predict(lower, top, C, V):
    xs, _ = forward(lower, V)
    W, b_h, b_v = top
    return R.predict(W, b_h, b_v, xs[-1], W.shape[0] - C)


def min_abs_pre(lower, V):
    """The smallest |pre-activation| over the relu layers of the stack on V (inf without one): a relu fixture is usable where no
    pre-activation sits at the kink."""
    _, pres = forward(lower, V)
    vals = [float(np.abs(p).min()) for p, (_, _, act) in zip(pres, lower) if act == ACT_RELU]
    return min(vals) if vals else float("inf")


def fine_tune(lower, top, C, V, y, batch_size, epochs, lr, momentum=0.0, weight_decay=0.0):
    """DBN.fine_tune(verbose = 0): contiguous batches, remainder last; every layer's sums at the weights the step started from, then
    every layer's update -- plain params += lr * sums, or with momentum / weight decay RBM's rule through a per-layer velocity (zero
    at the start): vel = mu vel + lr (g - weight_decay W); W += vel; biases without decay.  momentum: a number or a per-epoch list
    (its last value holds on).  A lower layer's visible bias is no parameter.  Parameters kept in float64 between the steps.
    Returns (lower, top, number of steps, the smallest |pre-activation| any relu layer met on the trajectory)."""
    lower = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64), act) for W, b, act in lower]
    top = tuple(np.array(x, dtype=np.float64) for x in top)
    sched = list(momentum) if isinstance(momentum, (list, tuple)) else [momentum]
    with_mom = weight_decay != 0.0 or any(m != 0.0 for m in sched)
    vel_l = [[np.zeros_like(W), np.zeros_like(b)] for W, b, _ in lower]
    vel_t = [np.zeros_like(x) for x in top]
    steps, margin = 0, float("inf")
    for epoch in range(epochs):
        mu = sched[min(epoch, len(sched) - 1)]
        for lo in range(0, V.shape[0], batch_size):
            Vb, yb = V[lo:lo + batch_size], y[lo:lo + batch_size]
            margin = min(margin, min_abs_pre(lower, Vb))
            s = grad(lower, top, C, Vb, yb)
            g_top = (s["top"]["dW"], s["top"]["db_h"], s["top"]["db_v"])
            if with_mom:
                for l, (W, b, act) in enumerate(lower):
                    vel_l[l][0] = mu * vel_l[l][0] + lr * (s["layers"][l]["dW"] - weight_decay * W)
                    vel_l[l][1] = mu * vel_l[l][1] + lr * s["layers"][l]["db_h"]
                    lower[l] = (W + vel_l[l][0], b + vel_l[l][1], act)
                vel_t[0] = mu * vel_t[0] + lr * (g_top[0] - weight_decay * top[0])
                vel_t[1] = mu * vel_t[1] + lr * g_top[1]
                vel_t[2] = mu * vel_t[2] + lr * g_top[2]
                top = tuple(p + v for p, v in zip(top, vel_t))
            else:
                lower = [(W + lr * sl["dW"], b + lr * sl["db_h"], act) for (W, b, act), sl in zip(lower, s["layers"])]
                top = tuple(p + lr * g for p, g in zip(top, g_top))
            steps += 1
    return lower, top, steps, margin


# ---- fixtures shared by the CPU and the GPU tier -------------------------------------------------------------------------------
def stack(sizes, n_top_hid, C, acts, seed=0, std=.3):
    """A stack sizes[0] -> sizes[1] -> ... under a (sizes[-1] + C) x n_top_hid label RBM, fp32 parameters ~ N(0, std)."""
    g = np.random.default_rng(4100 + seed)
    lower = [(g.normal(0, std, (a, b)).astype(np.float32), g.normal(0, std, b).astype(np.float32), act)
             for a, b, act in zip(sizes[:-1], sizes[1:], acts)]
    nv = sizes[-1] + C
    top = (g.normal(0, std, (nv, n_top_hid)).astype(np.float32), g.normal(0, std, n_top_hid).astype(np.float32),
           g.normal(0, std, nv).astype(np.float32))
    return lower, top


def batch(rows, n_vis, C, seed=0, binary=True):
    """V [rows, n_vis] fp32 (0/1, or N(0, 1) for Gaussian-mode bottoms) and labels y [rows]."""
    g = np.random.default_rng(4200 + seed)
    V = (g.random((rows, n_vis)) < .5).astype(np.float32) if binary else g.normal(0, 1, (rows, n_vis)).astype(np.float32)
    return V, g.integers(0, C, rows)


# The trajectory fixture of the GPU tier (test_gpu_backprop.py, item 5): 20 -> 12 -> 9 under a 9 + 3 -> 8 top, N = 50, batch 16
# (remainder 2), 2 epochs.  TRAJ_SEEDS: the seed per bottom activation for which no relu pre-activation of the WHOLE trajectory
# comes within RELU_MARGIN of zero (test_backprop_host.py asserts it, plain and with momentum).
TRAJ = dict(sizes=(20, 12, 9), n_top_hid=8, C=3, N=50, batch=16, epochs=2, lr=1e-2, momentum=[0.5, 0.9], weight_decay=1e-3)
RELU_MARGIN = 1e-3
TRAJ_SEEDS = {ACT_SIGMOID: 0, ACT_RELU: 5}


def traj_problem(act):
    """(lower, top, V, y) of the trajectory fixture with both lower layers of activation `act` (relu: real-valued data)."""
    T = TRAJ
    lower, top = stack(T["sizes"], T["n_top_hid"], T["C"], (act, act), seed=TRAJ_SEEDS[act], std=.3)
    V, y = batch(T["N"], T["sizes"][0], T["C"], seed=TRAJ_SEEDS[act], binary=act != ACT_RELU)
    return lower, top, V, y
