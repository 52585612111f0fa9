"""RBM with the class surface of the reference ``ku.ebm.RBM`` (reference ku/ebm/rbm.py:19-242),
driven by hand-written gfx950 HIP kernels through the C ABI of ``include/kurbm.h``.

What is kept verbatim from the reference: the constructor signature
``RBM(hps, output_dim, name=None, mode=MODE_VISIBLE_GAUSSIAN, **kwargs)`` (rbm.py:22), the hps
keys ``batch_size`` / ``epochs`` / ``lr`` (rbm.py:46,113,128), the methods ``build`` / ``call`` /
``transform`` / ``inv_transform`` / ``cal_free_energy`` / ``fit`` / ``compute_output_shape`` /
``get_config``, the attributes ``rbm_weight`` / ``hidden_bias`` / ``visible_bias``, the batch order
of ``fit`` (contiguous, unshuffled, remainder last: rbm.py:110-111, :211, :218), the update rules
(sums over the batch scaled by lr only: rbm.py:125-134) and the per-step score print
(rbm.py:225-234).  The TensorFlow graph machinery (placeholders, K.function) is gone.

Where the reference cannot run as written, the minimal repairs of SURVEY.md 8(a) apply (uniform
shape follows the probabilities, remainder-batch shape, list returns of K.function, ...).

Extensions, all off by default or reference-preserving: ``update_mode='fused'`` (one Gibbs chain
feeds all three updates; ``'reference_sequential'`` replays the reference's three chains),
``cd_k``, ``persistent`` chains, ``seed``, data-parallel training when torch.distributed is
initialised, ``verbose=0`` to skip the score passes, ``momentum`` / ``weight_decay`` (both 0 by
default: the reference's bare rule on the same kernels), ``n_labels`` (softmax label units: joint training on
[pixels | one-hot label], ``class_logits`` / ``predict_proba`` / ``predict``, ``sample(label=)``; 0 by default),
``objective`` / ``gen_weight`` (what a label RBM's ``fit`` climbs: ``'generative'`` by default, ``'discriminative'`` the exact
gradient of log p(y | v), ``'hybrid'`` both in one update).
"""
import collections
import time

import numpy as np
import torch

from .. import _lib
from . import ais, dp
from .engine import (CHAIN_BH, CHAIN_BV, CHAIN_SCORE, CHAIN_STRIDE, CHAIN_W, MODE_COMPLEX,
                     MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN, STREAM_GIBBS_V, STREAM_INV_TRANSFORM, STREAM_TRANSFORM,
                     DeviceMatrix, DeviceRBM, device_guard, hidden_site, resolve_device, visible_site)

_UPDATE_MODES = ("fused", "reference_sequential")
_OBJECTIVES = ("generative", "discriminative", "hybrid")


def _unwrap(x):
    """K.function takes and returns 1-element lists (rbm.py:89, :211, :233): accept both forms."""
    if isinstance(x, (list, tuple)):
        if len(x) != 1:
            raise ValueError("expected an array or a 1-element list of arrays")
        return x[0]
    return x


class _ScoreRing:
    """The per-step score of fit(verbose = 1) on its way from the device to stdout without a host synchronisation per
    step: each score is copied (asynchronously, on the stream that computed it) into a slot of a small pinned host ring,
    an event marks the copy, and a step's line is handed to `sink` once the step AFTER it has been queued -- by then its
    event has normally fired, so the host stays one step ahead of the device instead of waiting for every step."""

    def __init__(self, device, sink, depth=8):
        self.cuda = torch.device(device).type == "cuda"
        self.buf = torch.empty((depth, 4), dtype=torch.float32, pin_memory=self.cuda)
        self.events = [torch.cuda.Event() if self.cuda else None for _ in range(depth)]
        self.pending, self.head, self.depth, self.sink = collections.deque(), 0, depth, sink

    def push(self, score_dev, label):
        slot, self.head = self.head, (self.head + 1) % self.depth
        self.buf[slot, :1].copy_(score_dev.reshape(-1)[:1], non_blocking=True)
        if self.cuda:
            self.events[slot].record()
        self.pending.append((slot, label))
        while len(self.pending) > 1:
            self._pop()

    def _pop(self):
        slot, label = self.pending.popleft()
        if self.cuda:
            self.events[slot].synchronize()
        self.sink(float(self.buf[slot, 0]), label)

    def flush(self):
        while self.pending:
            self._pop()


class RBM(object):
    """Restricted Boltzmann machine trained by contrastive divergence on MI355X."""

    def __init__(self, hps, output_dim, name=None, mode=MODE_VISIBLE_GAUSSIAN, **kwargs):
        self.hps = hps
        self.output_dim = int(output_dim)
        self.name = name
        self.mode = mode
        if mode not in (MODE_VISIBLE_BERNOULLI, MODE_VISIBLE_GAUSSIAN):
            # MODE_COMPLEX is a TODO in the reference too (rbm.py:16, :68-70)
            raise ValueError("unsupported RBM mode %r" % (mode,))
        opt = lambda key, default: kwargs.pop(key, hps.get(key, default) if hasattr(hps, "get") else default)
        self.seed = int(opt("seed", 0))
        self.update_mode = opt("update_mode", "fused")
        if self.update_mode not in _UPDATE_MODES:
            raise ValueError("update_mode must be one of %s" % (_UPDATE_MODES,))
        self.cd_k = int(opt("cd_k", 1))
        self.persistent = bool(opt("persistent", False))
        # momentum and L2 weight decay, fused into the launch that applies the update (extension; 0 / 0 = the reference's bare rule,
        # through the same entry points as before):  vel <- mu vel + lr (g - weight_decay W); W <- W + vel (biases: no decay).
        # g = the batch SUMS, as lr multiplies sums (rbm.py:128) -- so weight_decay is on the scale of those sums: a mean-gradient
        # recipe's lambda (Hinton's guide: ~1e-4) times the batch size.  It is not rescaled by the row count (a remainder batch,
        # a data-parallel shard: the apply sees only the sum).  momentum: a float, or a sequence indexed by epoch whose last value
        # holds for every later epoch -- [0.5] * 5 + [0.9] is Hinton's schedule.
        mu = opt("momentum", 0.0)
        self.momentum = [float(m) for m in mu] if isinstance(mu, (list, tuple)) else float(mu)
        self.weight_decay = float(opt("weight_decay", 0.0))
        if isinstance(self.momentum, list) and not self.momentum:
            raise ValueError("momentum: an empty schedule")
        if any(not 0.0 <= m < 1.0 for m in (self.momentum if isinstance(self.momentum, list) else [self.momentum])):
            raise ValueError("momentum must be in [0, 1)")
        if not self.weight_decay >= 0.0:
            raise ValueError("weight_decay must be >= 0")
        # how the matrix products of fit() run (extension; storage, accumulation and results are fp32 in all):
        #   'fp32'  fp32 MFMA               'x3'  fp32 values as exact bf16 triples on the bf16 MFMA
        #   'bf16'  operands ROUNDED to bf16 (reduced precision, BASELINE.json config 5)
        #   'small' the whole CD-1 step in ONE launch (kurbm_cd_step_small; fp32 MFMA): the reference example's own sizes
        #   'auto'  (default) 'x3' at batch sizes >= 256 (tools/bench_fit.py, 784 x 1024, us per step fp32 / x3,
        #           end of round 3: batch 256 95 / 87, 512 102 / 87, 1024 122 / 95, 2048 194 / 105, 4096 341 / 129); below that
        #           'small' where it applies (CD-1 from the data, one GPU, no momentum and no weight decay: the one-launch kernel
        #           has neither, so with either term set 'auto' and 'small' take the five-launch paths, as they do for cd_k > 1), else 'fp32' 
        self.compute_dtype = str(opt("compute_dtype", "auto"))
        if self.compute_dtype not in ("fp32", "x3", "bf16", "small", "auto"):
            raise ValueError("compute_dtype must be 'fp32', 'x3', 'bf16', 'small' or 'auto'")
        # softmax label units (extension): the LAST n_labels visible units are one softmax group -- joint training on
        # [pixels | one-hot label], exact class posteriors (class_logits / predict_proba / predict), class-conditional samples
        # (sample(label=)).  include/kurbm.h states the model.  0 = an ordinary RBM, through the same calls as before.
        self.n_labels = int(opt("n_labels", 0))
        if self.n_labels != 0 and not 2 <= self.n_labels <= 64:
            raise ValueError("n_labels must be 0 or in [2, 64], got %d" % self.n_labels)
        if self.n_labels and mode != MODE_VISIBLE_BERNOULLI:
            raise ValueError("label units need MODE_VISIBLE_BERNOULLI: the label block is a softmax group among Bernoulli visibles")
        # what fit() of a label RBM climbs (extension; Larochelle & Bengio 2008): 'generative' (default) log p(v, y) by CD, exactly the
        # calls of before; 'discriminative' the exact gradient of log p(y | v) -- no chain, no random number; 'hybrid'
        # log p(y | v) + gen_weight log p(v, y), ONE update per batch from both gradients at the same weights.  include/kurbm.h
        # ("discriminative and hybrid training") states the gradient.  gen_weight is read by 'hybrid' only (the paper's order: 0.01).
        self.objective = str(opt("objective", "generative"))
        if self.objective not in _OBJECTIVES:
            raise ValueError("objective must be one of %s, got %r" % (_OBJECTIVES, self.objective))
        self.gen_weight = float(opt("gen_weight", 0.01))
        if self.objective != "generative" and not self.n_labels:
            raise ValueError("objective %r needs a label RBM (n_labels > 0)" % self.objective)
        if self.objective == "hybrid" and not (self.gen_weight > 0.0 and np.isfinite(self.gen_weight)):
            raise ValueError("objective 'hybrid' needs a finite gen_weight > 0, got %r" % self.gen_weight)
        self.list_returns = bool(kwargs.pop("ku_compat_list_returns", True))
        self._device_arg = kwargs.pop("device", None)
        self._init_weights = kwargs.pop("weights", None)
        self._kwargs = kwargs          # remaining Keras Layer kwargs (dtype, trainable, ...) are kept for get_config
        self.built = False
        self.input_shape = None
        self.output_shape = None
        self._dev = None               # DeviceRBM
        self._update_count = 0         # `step` of the RNG contract for fit()
        self._call_count = 0           # `step` of the RNG contract for transform / inv_transform / call
        self._v_chain = None           # persistent fantasy particles
        self._planes = None            # engine.ResidentPlanes of the data matrix during an x3 fit()
        self._epochs_done = 0          # epochs this object has trained: the index into a momentum schedule
        self._mom_kw = {}              # the `momentum=` keyword of this epoch's engine calls; empty with both terms 0
        self.last_scores = []
        self.last_ais = None           # what the last log_partition() found (and the update count it was valid at)
        self._ais_at = -1
        self._chains_used = 0          # Gibbs chains handed out by gibbs() / sample() so far (a multiple of 4): their chain0

    # ------------------------------------------------------------------ build ----------
    def build(self, input_shape):
        """Create W ~ U(-0.05, 0.05) [n_vis, n_hid], b_h, b_v on the device (rbm.py:29-40)."""
        n_vis = int(input_shape[1])
        if self.n_labels and n_vis <= self.n_labels:
            raise ValueError("%d visible units leave no pixel beside %d label units" % (n_vis, self.n_labels))
        if self._init_weights is not None:
            W, b_h, b_v = self._init_weights
        else:
            g = np.random.default_rng(self.seed)
            W = g.uniform(-0.05, 0.05, size=(n_vis, self.output_dim)).astype(np.float32)
            b_h = g.uniform(-0.05, 0.05, size=(self.output_dim,)).astype(np.float32)
            b_v = g.uniform(-0.05, 0.05, size=(n_vis,)).astype(np.float32)
        W = np.asarray(W, dtype=np.float32)
        if W.shape != (n_vis, self.output_dim):
            raise ValueError("weights have shape %s, expected %s" % (W.shape, (n_vis, self.output_dim)))
        self._dev = DeviceRBM(W, b_h, b_v, resolve_device(self._device_arg))
        self.input_shape = (None, n_vis)
        self.output_shape = (None, self.output_dim)
        self.built = True

    def _ensure_built(self, n_cols):
        if not self.built:
            self.build((None, n_cols))

    # ------------------------------------------------------------------ variables ------
    @property
    def rbm_weight(self):
        return self._dev.get_weights()[0]

    @rbm_weight.setter
    def rbm_weight(self, W):
        self._dev.set_weights(W=W)

    @property
    def hidden_bias(self):
        return self._dev.get_weights()[1]

    @hidden_bias.setter
    def hidden_bias(self, b):
        self._dev.set_weights(b_h=b)

    @property
    def visible_bias(self):
        return self._dev.get_weights()[2]

    @visible_bias.setter
    def visible_bias(self, b):
        self._dev.set_weights(b_v=b)

    def get_weights(self):
        """[rbm_weight, rbm_hidden_bias, rbm_visible_bias] -- unlike the reference, the visible bias
        is included (there it is a bare K.variable and is silently dropped: rbm.py:38-40)."""
        return list(self._dev.get_weights())

    def set_weights(self, weights):
        W, b_h = weights[0], weights[1]
        b_v = weights[2] if len(weights) > 2 else None
        self._dev.set_weights(W, b_h, b_v)

    # ------------------------------------------------------------------ forward passes --
    @staticmethod
    def _n_cols(x):
        x = _unwrap(x)
        return x.cols if isinstance(x, DeviceMatrix) else x.shape[1]

    def _as_device(self, x):
        """(DeviceMatrix, kind): kind = "device" for a DeviceMatrix, the input's torch.device for a tensor, "numpy"."""
        x = _unwrap(x)
        if isinstance(x, DeviceMatrix):
            return x, "device"
        kind = x.device if isinstance(x, torch.Tensor) else "numpy"
        dev = self._dev.device if self._dev is not None else resolve_device(self._device_arg)
        with device_guard(dev):
            return DeviceMatrix.from_host(x, dev), kind

    def _ret(self, m, kind, as_list):
        """Results go back where the input came from: a DeviceMatrix as is, a tensor on the input tensor's device,
        a numpy array on the host (the K.function convention of the reference)."""
        if kind == "device":
            out = m
        elif isinstance(kind, torch.device):
            out = m.view().to(kind)
        else:
            out = m.to_numpy()
        return [out] if as_list else out

    def _half(self, direction, x, act, noise, stream_id):
        if x.rows == 0:
            # an empty batch yields an empty result (K.function on a [0, n] feed does); the call still counts for the RNG
            self._call_count += 1
            n_out = self._dev.n_hid if direction == "vh" else self._dev.n_vis
            return DeviceMatrix.zeros(0, n_out, self._dev.device)
        # large inputs (a whole data set between DBN layers) go through the x3 kernels too
        if self._large(x.rows):
            out = self._dev.half_step_bf16(direction, x, x.rows, act, noise, self.seed, stream_id, self._call_count, pieces=3,
                                           want_prob=False, want_u=False)
        else:
            out = self._dev.half_step(direction, x, x.rows, 0, act, noise, self.seed, stream_id, self._call_count)
        self._call_count += 1
        return out["sample"]

    def _large(self, rows):
        """Inference-side calls of at least 1024 rows use the x3 kernels (as training does from that batch size on)."""
        return self.compute_dtype in ("auto", "x3") and rows >= 1024

    def _sample_hidden(self, x):
        act, noise = hidden_site(self.mode)
        return self._half("vh", x, act, noise, STREAM_TRANSFORM)

    def _sample_visible(self, h):
        act, noise = visible_site(self.mode)
        return self._half("hv", h, act, noise, STREAM_INV_TRANSFORM)

    def transform(self, v):
        """Sampled hidden states of v (transform_func, rbm.py:88-89 -> :46-48 / :58-60)."""
        self._ensure_built(self._n_cols(v))
        x, kind = self._as_device(v)
        return self._ret(self._sample_hidden(x), kind, self.list_returns and kind != "device")

    def inv_transform(self, h):
        """Sampled visible states of h (inv_transform_func, rbm.py:91-92 -> :52-54 / :64-67)."""
        if not self.built:
            raise ValueError("inv_transform needs a built RBM (call build / fit / transform first)")
        x, kind = self._as_device(h)
        step = self._call_count
        out = self._sample_visible(x)
        if self.n_labels and x.rows > 0:
            # the label block is one softmax draw (the label site, same stream and call counter), not n_labels Bernoulli ones
            self._dev.label_sample(x, out, self.n_labels, self.seed, STREAM_INV_TRANSFORM, step)
        return self._ret(out, kind, self.list_returns and kind != "device")

    def call(self, x):
        """The layer's forward pass: stochastic hidden features (rbm.py:80-86)."""
        self._ensure_built(self._n_cols(x))
        xd, kind = self._as_device(x)
        return self._ret(self._sample_hidden(xd), kind, False)

    __call__ = call

    def cal_free_energy(self, v):
        """F(v) = -(v.b_v + sum_j softplus((v.W + b_h)_j))   (free_energy_func, rbm.py:97-98 -> :73-76)."""
        self._ensure_built(self._n_cols(v))
        x, kind = self._as_device(v)
        if x.rows == 0:
            F = torch.empty(0, dtype=torch.float32, device=self._dev.device)
        else:
            F = self._dev.free_energy(x, x.rows, compute="x3" if self._large(x.rows) else None)
        if kind == "device":
            return F
        if isinstance(kind, torch.device):          # torch input: the result goes back to the input's device
            F = F.to(kind)
            return [F] if self.list_returns else F
        F = F.cpu().numpy()
        return [F] if self.list_returns else F

    def compute_output_shape(self, input_shape):
        return (input_shape[0], self.output_dim)          # rbm.py:94-95

    # ------------------------------------------------------------------ likelihood -------
    def _check_likelihood(self, what, label=None):
        if label is not None and label != "free":
            raise ValueError("label= of %s is None or 'free', got %r" % (what, label))
        if label is not None and not self.n_labels:
            raise ValueError("label= needs a label RBM (n_labels > 0)")
        if self.n_labels and label is None:
            raise ValueError("%s of a label RBM is that of the joint model p(v, y): pass label='free' (the AIS run then samples "
                             "the label block at its softmax site)" % what)
        if self.mode != MODE_VISIBLE_BERNOULLI:
            raise ValueError("%s is defined for MODE_VISIBLE_BERNOULLI only: in MODE_VISIBLE_GAUSSIAN the hidden site is a "
                             "thresholded relu (rbm.py:58-59), not the Bernoulli unit of an energy model this estimator is valid for"
                             % what)

    def _check_built(self, what):
        if not self.built:
            raise ValueError("%s needs a built RBM (call build / fit / transform first)" % what)

    def log_partition(self, n_chains=512, betas=1000, base_rates=None, seed=None, method="ais", label=None):
        """log Z of the model (extension; the reference has no likelihood estimate).

        method 'ais': annealed importance sampling (Salakhutdinov & Murray 2008) from the base-rate model to this one, n_chains
        chains on the device in one library call (kurbm_ais_run).  betas: the number of annealing steps of a linear schedule, or
        the schedule itself (0 ... 1, strictly increasing; ais.beta_schedule(n, 'three_stage') is the paper's).  base_rates: None
        (b_A = 0: the uniform base model), a data matrix [rows, n_vis] (-> ais.base_rate_bias, the usual choice for a trained
        model) or a bias vector [n_vis].  seed: of the chains' draws (default: the RBM's).
        method 'exact': enumeration (ais.exact_log_partition; at most 24 units on the smaller side).
        Returns a float and fills self.last_ais = {log_z, stderr, log_z0, logw, n_chains, n_betas}.  The fit / transform counters
        and the weights are not touched.
        label='free' (label RBM only, and required there): log Z of the joint model p(v, y) over [pixels | one-hot] -- the AIS
        chains sample the label block at its softmax site (kurbm_ais_run_labels), the base model of the block is categorical
        (ais.base_rate_bias(V, n_labels=C)), and 'exact' enumerates pixels x classes or the hidden side."""
        self._check_likelihood("log_partition", label)
        C_lab = self.n_labels if label == "free" else 0
        if method not in ("ais", "exact"):
            raise ValueError("method must be 'ais' or 'exact', got %r" % (method,))
        if method == "ais":          # (arguments first: a bad schedule is refused whether or not the RBM is built)
            if isinstance(betas, (int, np.integer)) and not isinstance(betas, bool):
                if betas < 1:
                    raise ValueError("betas: a schedule needs at least one step, got %d" % betas)
                betas = ais.beta_schedule(int(betas))
            else:
                betas = ais.check_schedule(betas)
            n_chains = int(n_chains)
            if n_chains < 1:
                raise ValueError("n_chains must be positive")
        self._check_built("log_partition")
        if method == "exact":
            W, b_h, b_v = self._dev.get_weights()
            log_z = ais.exact_log_partition(W, b_h, b_v, n_labels=C_lab) if C_lab else ais.exact_log_partition(W, b_h, b_v)
            self.last_ais = {"log_z": log_z, "stderr": 0.0, "log_z0": None, "logw": None, "n_chains": 0, "n_betas": 0}
            self._ais_at = self._update_count
            return log_z
        d = self._dev
        if base_rates is None:
            b_a = np.zeros(d.n_vis, np.float64)
        else:
            b_a = np.asarray(base_rates, dtype=np.float64)
            b_a = (ais.base_rate_bias(b_a, n_labels=C_lab) if C_lab else ais.base_rate_bias(b_a)) if b_a.ndim == 2 else b_a.reshape(-1)
            if b_a.size != d.n_vis:
                raise ValueError("base_rates has %d columns, the RBM has %d visible units" % (b_a.size, d.n_vis))
        b_a = b_a.astype(np.float32)          # what the device anneals from; log Z_0 is of exactly these values
        seed = self.seed if seed is None else int(seed)
        if C_lab:
            logw, _ = d.ais_run(betas, n_chains, base_bias=b_a, seed=seed, n_labels=C_lab)
        else:
            logw, _ = d.ais_run(betas, n_chains, base_bias=b_a, seed=seed)
        logw = logw.cpu().numpy()
        log_z, stderr, z0 = ais.estimate(logw, b_a, d.n_hid, n_labels=C_lab) if C_lab else ais.estimate(logw, b_a, d.n_hid)
        self.last_ais = {"log_z": log_z, "stderr": stderr, "log_z0": z0, "logw": logw, "n_chains": n_chains, "n_betas": int(betas.size)}
        self._ais_at = self._update_count
        return log_z

    def log_likelihood(self, V, y=None, log_z=None, label=None, **ais_kwargs):
        """Mean log p(v) = -F(v) - log Z over the rows of V.  log_z: given, else the one log_partition cached (self.last_ais; a
        fit() since then discards it), else log_partition(**ais_kwargs) is run first.  F(v) is cal_free_energy's device path.
        label='free' (label RBM only, and required there) -- the joint model:
          V n_pix wide with integer labels y, or n_vis wide with a one-hot block: mean log p(v, y) = -F([v | y]) - log Z;
          V n_pix wide without y: the mean marginal log p(v) = v.b_v[:n_pix] + logsumexp_c class_logits(v) - log Z.
        V is validated before any log Z is computed."""
        self._check_likelihood("log_likelihood", label)
        if y is not None and label != "free":
            raise ValueError("y= needs a label RBM and label='free'")
        if label == "free":
            return self._log_likelihood_labels(V, y, log_z, ais_kwargs)
        if log_z is None:
            cached = self.last_ais is not None and self._ais_at == self._update_count and not ais_kwargs
            log_z = self.last_ais["log_z"] if cached else self.log_partition(**ais_kwargs)
        self._check_built("log_likelihood")
        x, _ = self._as_device(V)
        if x.cols != self._dev.n_vis:
            raise ValueError("V has %d columns, the RBM has %d visible units" % (x.cols, self._dev.n_vis))
        if x.rows == 0:
            raise ValueError("log_likelihood of an empty matrix")
        F = self._dev.free_energy(x, x.rows, compute="x3" if self._large(x.rows) else None)
        return float(-F.double().mean().item() - float(log_z))

    def _block_classes(self, x, what):
        """The classes of the one-hot label blocks of DeviceMatrix x [rows, n_vis] (a device int64 tensor), or ValueError."""
        blk = x.view()[:, self._n_pix():]
        if not bool((((blk == 0) | (blk == 1)).all(dim=1) & (blk.sum(dim=1) == 1)).all().item()):
            raise ValueError("%s: the label block of a label RBM must be one-hot (exactly one of its %d units at 1, the others 0)"
                             % (what, self.n_labels))
        return blk.argmax(dim=1)

    def _log_likelihood_labels(self, V, y, log_z, ais_kwargs):
        self._check_built("log_likelihood")
        d, n_pix = self._dev, self._n_pix()
        x, _ = self._as_device(V)
        if x.cols not in (n_pix, d.n_vis):
            raise ValueError("V has %d columns, expected %d (pixels) or %d (pixels and labels)" % (x.cols, n_pix, d.n_vis))
        if x.rows == 0:
            raise ValueError("log_likelihood of an empty matrix")
        if x.cols == d.n_vis:
            if y is not None:
                raise ValueError("V carries a label block already: pass the pixels alone with y=")
            self._block_classes(x, "log_likelihood")
        elif y is not None:
            x = self._with_label(x, y)
        if log_z is None:
            cached = self.last_ais is not None and self._ais_at == self._update_count and not ais_kwargs
            log_z = self.last_ais["log_z"] if cached else self.log_partition(label="free", **ais_kwargs)
        if x.cols == d.n_vis:          # joint: the free energy of the joined matrix is -log p*(v, y)
            F = d.free_energy(x, x.rows)
            return float(-F.double().mean().item() - float(log_z))
        logits, _ = d.class_logits(x, self.n_labels, want_prob=False)
        with device_guard(d.device):
            lse = torch.logsumexp(logits.view().double(), dim=1)
            lin = x.view().double() @ d.b_v[:n_pix].double()
        return float((lin + lse).mean().item() - float(log_z))

    # ------------------------------------------------------------------ sampling ---------
    def _take_chains(self, n):
        """Fresh chain indices for n chains: the count handed out so far (kept a multiple of 4, as the draws' row0 must be)."""
        chain0 = self._chains_used
        self._chains_used = (chain0 + int(n) + 3) // 4 * 4
        return chain0

    def _gibbs_out(self, out, prob, n_rows, kind, return_prob):
        cut = lambda m: m if m.rows == n_rows else DeviceMatrix(m.t, n_rows, m.cols, m.ld)
        v = self._ret(cut(out), kind, False)
        return (v, self._ret(cut(prob), kind, False)) if return_prob else v

    # ------------------------------------------------------------------ label units -------
    def _n_pix(self):
        return self._dev.n_vis - self.n_labels

    def _labels(self, y, rows):
        """Integer labels in [0, n_labels) as a host int64 array [rows]; a single integer stands for every row."""
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if y.dtype.kind not in "iu":
            raise ValueError("labels must be integers in [0, %d)" % self.n_labels)
        y = np.full(rows, int(y), np.int64) if y.ndim == 0 else y.reshape(-1).astype(np.int64)
        if y.size != rows:
            raise ValueError("%d labels for %d rows" % (y.size, rows))
        if y.size and (y.min() < 0 or y.max() >= self.n_labels):
            raise ValueError("labels must be integers in [0, %d)" % self.n_labels)
        return y

    def _with_label(self, x, y):
        """A new DeviceMatrix [rows, n_vis]: the pixel columns of x (n_pix or n_vis wide) and the one-hot block of labels y."""
        d, n_pix = self._dev, self._n_pix()
        if x.cols not in (n_pix, d.n_vis):
            raise ValueError("input has %d columns, expected %d (pixels) or %d (pixels and labels)" % (x.cols, n_pix, d.n_vis))
        y = self._labels(y, x.rows)
        with device_guard(d.device):
            m = DeviceMatrix.zeros(x.rows, d.n_vis, d.device)
            if x.rows:
                m.t[:x.rows, :n_pix].copy_(x.t[:x.rows, :n_pix])
                m.t[torch.arange(x.rows, device=d.device), n_pix + torch.from_numpy(y).to(d.device)] = 1.0
        return m

    def join(self, V, y):
        """[pixels | one-hot label]: V [N, n_pix] and integer labels y [N] in [0, n_labels) as one fp32 host array [N, n_pix +
        n_labels], the layout fit(), transform() and gibbs() of a label RBM take."""
        if not self.n_labels:
            raise ValueError("join needs a label RBM (n_labels > 0)")
        V = _unwrap(V)
        V = V.detach().cpu().numpy() if isinstance(V, torch.Tensor) else (V.to_numpy() if isinstance(V, DeviceMatrix) else np.asarray(V))
        if V.ndim != 2:
            raise ValueError("expected a 2-d array, got shape %s" % (V.shape,))
        y = self._labels(y, V.shape[0])
        out = np.zeros((V.shape[0], V.shape[1] + self.n_labels), np.float32)
        out[:, :V.shape[1]] = V
        out[np.arange(V.shape[0]), V.shape[1] + y] = 1.0
        return out

    def _label_clamp(self, clamp, label):
        """The clamp mask of a Gibbs run on a label RBM, and whether its block is FREE.  Clamped block (label a class, or None with
        a clamp that covers the block): the whole label block joined with the caller's mask, through kurbm_gibbs_run.
        label='free': the block is sampled at its softmax site (kurbm_gibbs_run_labels) and the mask holds the caller's pixels; a
        clamp that covers the WHOLE block is the clamped run again, one that covers part of it is refused."""
        d, n_pix = self._dev, self._n_pix()
        from .engine import clamp_mask
        m = clamp_mask(clamp, d.n_vis) if clamp is not None else np.zeros(d.n_vis, np.uint8)
        if isinstance(label, str):
            if label != "free":
                raise ValueError("label= is a class, one class per chain, or 'free', got %r" % (label,))
            if not m[n_pix:].any():
                return (m.astype(bool) if m.any() else None), True
            if not m[n_pix:].all():
                raise ValueError("label='free': the clamp covers part of the label block; clamp all of it or none of it")
            return m.astype(bool), False
        if label is None and not m[n_pix:].all():
            raise ValueError("a label RBM samples with its label block clamped: pass label= (a class, or label='free' to sample "
                             "the block at its softmax site), or a clamp that covers the whole block and an init that carries it")
        m[n_pix:] = 1
        return m.astype(bool), False

    def _free_block_start(self, x, chain0, seed):
        """A new DeviceMatrix [rows, n_vis]: the pixels of x (n_pix wide) and a one-hot block drawn from softmax(b_v[n_pix:]) with
        the uniforms u(chain0 + row, n_pix) of site STREAM_GIBBS_V at step 0 -- the label site's rule (first class whose running
        fp32 sum exceeds u, else the last).  Host tensor arithmetic, as _start_chains."""
        d, n_pix, C = self._dev, self._n_pix(), self.n_labels
        with device_guard(d.device):
            u = d.philox_uniform(x.rows, n_pix + 1, seed, STREAM_GIBBS_V, 0, row0=chain0).view()[:, n_pix]
            cum = torch.cumsum(torch.softmax(d.b_v[n_pix:].float(), dim=0), dim=0)
            y = torch.clamp((u.reshape(-1, 1) >= cum.reshape(1, -1)).sum(dim=1), max=C - 1)
            m = DeviceMatrix.zeros(x.rows, d.n_vis, d.device)
            m.t[:x.rows, :n_pix].copy_(x.t[:x.rows, :n_pix])
            m.t[torch.arange(x.rows, device=d.device), n_pix + y] = 1.0
        return m

    def _class_logits(self, V):
        self._check_built("class_logits")
        if not self.n_labels:
            raise ValueError("class_logits needs a label RBM (n_labels > 0)")
        x, kind = self._as_device(V)
        d = self._dev
        if x.cols not in (self._n_pix(), d.n_vis):
            raise ValueError("V has %d columns, expected %d (pixels) or %d (pixels and labels)" % (x.cols, self._n_pix(), d.n_vis))
        if x.rows == 0:
            e = DeviceMatrix.zeros(0, self.n_labels, d.device)
            return e, e, kind
        logits, prob = d.class_logits(x, self.n_labels)
        return logits, prob, kind

    def class_logits(self, V):
        """logit_c = b_v[n_pix + c] + sum_j softplus((v.W[:n_pix] + b_h)_j + W[n_pix + c, j]) for the pixels of V, [N, n_labels]:
        -F(v, y = c) up to the class-independent term v.b_v.  V has n_pix or n_vis columns (a label block is ignored).  Two
        launches (kurbm_class_logits).  One array, where V came from."""
        logits, _, kind = self._class_logits(V)
        return self._ret(logits, kind, False)

    def predict_proba(self, V):
        """The exact class posterior p(y | v) = softmax(class_logits), [N, n_labels]; rows sum to 1."""
        _, prob, kind = self._class_logits(V)
        return self._ret(prob, kind, False)

    def predict(self, V):
        """argmax_c p(y = c | v) as integers [N] (a host array, or a tensor where V came from)."""
        logits, _, kind = self._class_logits(V)
        y = logits.view().argmax(dim=1)
        return y.cpu().numpy() if kind == "numpy" else (y if kind == "device" else y.to(kind))

    def gibbs(self, v, n_steps=1, clamp=None, return_prob=False, seed=None, label=None):
        """The chains after n_steps Gibbs sweeps from the rows of v (extension; the reference has one half step per call):
        h ~ p(h | v), v ~ p(v | h) at the sites of transform / inv_transform for this mode, in ONE library call
        (kurbm_gibbs_run).  clamp: a boolean mask [n_vis] or a list of unit indices -- those units keep v's values (a
        conditional completion).  return_prob: also the probabilities (Gaussian visibles: the means) the last states were drawn
        from, as (samples, probs).  seed: of the draws (default: the RBM's).  Every call takes fresh chain indices, so two calls
        never reuse draws, and a run is reproducible from (seed, the number of chains handed out before it).  The fit / transform
        counters, the weights and the cached AIS result are not touched.  Results go back where v came from, as one array.
        label (label RBM only): a class, or one per row -- the sweeps keep that one-hot block; or 'free' -- the block is drawn at
        its softmax site every sweep (kurbm_gibbs_run_labels): v is n_vis wide with a one-hot block, or the pixels alone (the block
        then starts as sample(init=None) starts it), and clamp may cover pixels: (y, h | clamped pixels)."""
        self._check_built("gibbs")
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        x, kind = self._as_device(v)
        d = self._dev
        if label is not None and not self.n_labels:
            raise ValueError("label= needs a label RBM (n_labels > 0)")
        free = False
        if self.n_labels:
            # label RBM: the chains start from the one-hot block of `label` (v: pixels, or pixels and a block that is replaced) and
            # keep it -- class-conditional sweeps through the same kurbm_gibbs_run; label='free' samples the block
            clamp, free = self._label_clamp(clamp, label)
            if label is not None and not isinstance(label, str) and x.rows > 0:
                x = self._with_label(x, label)
        seed = self.seed if seed is None else int(seed)
        if free:
            if x.cols not in (self._n_pix(), d.n_vis):
                raise ValueError("v has %d columns, expected %d (pixels) or %d (pixels and labels)" % (x.cols, self._n_pix(), d.n_vis))
            if x.rows == 0:
                raise ValueError("gibbs on an empty matrix")
            if x.cols == d.n_vis:
                self._block_classes(x, "gibbs(label='free')")
            chain0 = self._take_chains(x.rows)
            if x.cols != d.n_vis:        # pixels alone: the block starts as sample(init=None) starts it
                x = self._free_block_start(x, chain0, seed)
            out, prob = d.gibbs_run(x, burn_in=n_steps, thin=1, n_keep=1, chain0=chain0, seed=seed, mode=self.mode, clamp=clamp,
                                    want_prob=bool(return_prob), n_labels=self.n_labels)
            return self._gibbs_out(out, prob, x.rows, kind, return_prob)
        if x.cols != d.n_vis:
            raise ValueError("v has %d columns, the RBM has %d visible units" % (x.cols, d.n_vis))
        if x.rows == 0:
            raise ValueError("gibbs on an empty matrix")
        out, prob = d.gibbs_run(x, burn_in=n_steps, thin=1, n_keep=1, chain0=self._take_chains(x.rows),
                                seed=seed, mode=self.mode, clamp=clamp, want_prob=bool(return_prob))
        return self._gibbs_out(out, prob, x.rows, kind, return_prob)

    def _start_chains(self, n_chains, chain0, seed):
        """v_0 of fresh chains: [u < sigmoid(b_v)] (Bernoulli visibles; u = the Philox uniforms of site STREAM_GIBBS_V at step 0,
        the sweep before the first) or b_v itself (Gaussian visibles).  Elementwise device arithmetic; no kernel of its own."""
        d = self._dev
        with device_guard(d.device):
            m = DeviceMatrix.zeros(n_chains, d.n_vis, d.device)
            if self.mode == MODE_VISIBLE_GAUSSIAN:
                m.view().copy_(d.b_v.reshape(1, -1).expand(n_chains, d.n_vis))
            else:
                u = d.philox_uniform(n_chains, d.n_vis, seed, STREAM_GIBBS_V, 0, row0=chain0)
                m.view().copy_((u.view() < torch.sigmoid(d.b_v).reshape(1, -1)).to(torch.float32))
                m.bf16_exact = m.binary = True
        return m

    def sample(self, n_samples, n_chains=None, burn_in=1000, thin=100, init=None, clamp=None, return_prob=False, seed=None, label=None):
        """n_samples draws from the model by Gibbs sampling (extension), [n_samples, n_vis].  n_chains (default n_samples:
        independent chains, one kept sample each) chains run burn_in sweeps; with fewer chains each keeps ceil(n_samples /
        n_chains) states `thin` sweeps apart, and the first n_samples rows in (kept, chain) order are returned.  init: the chains'
        start [n_chains, n_vis]; None starts them at [u < sigmoid(b_v)] (Bernoulli visibles) or b_v (Gaussian).  clamp (mask or
        index list, see gibbs) needs init, which carries the clamped values.  return_prob, seed, the chain bookkeeping and what
        is left untouched: as gibbs.  The result is a host array, or goes where init came from.
        label (label RBM only): a class, or one class per chain -- the chains start from that one-hot block and keep it
        (class-conditional samples); init may then hold the pixels alone.  label='free': joint samples (v, y) -- the block is
        drawn at its softmax site every sweep (kurbm_gibbs_run_labels); init=None starts it one-hot from softmax(b_v[n_pix:]), an
        init must carry a one-hot block, and clamp may cover pixels (y, h | clamped pixels).  Without label= a label RBM refuses
        to sample."""
        out, prob, kind = self._sample(n_samples, n_chains, burn_in, thin, init, clamp, return_prob, seed, label)
        return self._gibbs_out(out, prob, int(n_samples), kind, return_prob)

    def _sample(self, n_samples, n_chains, burn_in, thin, init, clamp, return_prob, seed, label=None):
        """sample() up to the device results: (samples, probs or None -- DeviceMatrix [n_keep * n_chains, n_vis] -- and where
        init came from).  DBN.sample takes the top RBM's states from here without a trip through the host."""
        self._check_built("sample")
        n_samples = int(n_samples)
        n_chains = n_samples if n_chains is None else int(n_chains)
        burn_in, thin = int(burn_in), int(thin)
        if n_samples < 1 or n_chains < 1:
            raise ValueError("n_samples and n_chains must be positive")
        if burn_in < 1 or thin < 1:
            raise ValueError("burn_in and thin must be >= 1")
        if clamp is not None and init is None:
            raise ValueError("clamp needs init: it carries the clamped values")
        if label is not None and not self.n_labels:
            raise ValueError("label= needs a label RBM (n_labels > 0)")
        d = self._dev
        free = False
        if self.n_labels:
            clamp, free = self._label_clamp(clamp, label)
            if isinstance(label, str):
                label = None          # ('free', or a clamp over the whole block with an init that carries it)
            if label is not None:
                label = self._labels(label, n_chains)
        seed = self.seed if seed is None else int(seed)
        kind = "numpy"
        if init is not None:
            x, kind = self._as_device(init)
            if label is not None and x.rows == n_chains and x.cols == self._n_pix():
                x = self._with_label(x, label)
            pix_only = free and x.rows == n_chains and x.cols == self._n_pix()     # the block then starts as with init=None
            if not pix_only and (x.cols != d.n_vis or x.rows != n_chains):
                raise ValueError("init has shape (%d, %d), expected (%d, %d)" % (x.rows, x.cols, n_chains, d.n_vis))
            if free and not pix_only:
                self._block_classes(x, "sample(label='free')")
        chain0 = self._take_chains(n_chains)
        if init is not None and free and x.cols != d.n_vis:
            x = self._free_block_start(x, chain0, seed)
        if init is None:
            x = self._start_chains(n_chains, chain0, seed)
            if free:       # the Bernoulli draws of the block's columns are replaced by ONE categorical draw per chain
                x = self._free_block_start(DeviceMatrix(x.t, x.rows, self._n_pix(), x.ld), chain0, seed)
                x.bf16_exact = x.binary = True
        if label is not None:
            x = self._with_label(x, label)      # (a copy: the caller's init is never written)
        n_keep = -(-n_samples // n_chains)
        if free:
            out, prob = d.gibbs_run(x, burn_in=burn_in, thin=thin, n_keep=n_keep, chain0=chain0, seed=seed, mode=self.mode,
                                    clamp=clamp, want_prob=bool(return_prob), n_labels=self.n_labels)
        else:
            out, prob = d.gibbs_run(x, burn_in=burn_in, thin=thin, n_keep=n_keep, chain0=chain0, seed=seed, mode=self.mode,
                                    clamp=clamp, want_prob=bool(return_prob))
        return out, prob, kind

    def _probs(self, direction, x, act):
        d = self._dev
        if x.rows == 0:
            return DeviceMatrix.zeros(0, d.n_hid if direction == "vh" else d.n_vis, d.device)
        if self._large(x.rows):
            return d.half_step_bf16(direction, x, x.rows, act, _lib.NOISE_NONE, 0, 0, 0, pieces=3, want_prob=True, want_u=False)["prob"]
        return d.half_step(direction, x, x.rows, 0, act, _lib.NOISE_NONE, 0, 0, 0, want_sample=False, want_prob=True)["prob"]

    def hidden_probs(self, v):
        """The activated hidden values of v without a draw -- sigmoid(v.W + b_h), or relu(v.W + b_h) with Gaussian visibles: the
        deterministic counterpart of transform (mean-field features).  No RNG counter is consumed.  One array, where v came from."""
        self._ensure_built(self._n_cols(v))
        x, kind = self._as_device(v)
        return self._ret(self._probs("vh", x, hidden_site(self.mode)[0]), kind, False)

    def visible_probs(self, h):
        """The activated visible values of h without a draw -- sigmoid(h.W^T + b_v), or the mean h.W^T + b_v of Gaussian visibles."""
        self._check_built("visible_probs")
        x, kind = self._as_device(h)
        return self._ret(self._probs("hv", x, visible_site(self.mode)[0]), kind, False)

    # ------------------------------------------------------------------ training --------
    def _score(self, Vd, lo, rows, step):
        """mean |F(v) - F(v')| with v' a fresh one-step reconstruction (rbm.py:225-233), as a DEVICE tensor (element 0):
        the launches are queued behind the update and nothing is read back here -- fit() prints a step's line when its
        score has landed in pinned host memory (_ScoreRing), so the reference's default verbose = 1 costs no host
        synchronisation per step."""
        d = self._dev
        base = CHAIN_SCORE * CHAIN_STRIDE
        if self.n_labels:
            # label RBM: the reconstruction's label block is drawn by the label site (same site and step as its pixels)
            act_h, noise_h = hidden_site(self.mode)
            act_v, noise_v = visible_site(self.mode)
            fe = d.free_energy(Vd, rows, lo)
            h = d.half_step("vh", Vd, rows, lo, act_h, noise_h, self.seed, base + 0, step)["sample"]
            v1 = d.half_step("hv", h, rows, 0, act_v, noise_v, self.seed, base + 1, step)["sample"]
            d.label_sample(h, v1, self.n_labels, self.seed, base + 1, step)
            fe_p = d.free_energy(v1, rows, 0)
            return (fe - fe_p).abs().mean().reshape(1)
        if self._large(rows):
            # one library call on the x3 kernels: same draws (chain CHAIN_SCORE, sites 0 and 1), products on the bf16 pieces
            return d.score_x3(Vd, rows, lo, self.seed, step, self.mode, CHAIN_SCORE, planes=self._planes)
        if self._compute() == "small" and rows <= 512:
            # small RBMs: the whole score in one launch, as their step is (same draws)
            return d.score_small(Vd, rows, lo, self.seed, step, self.mode, CHAIN_SCORE)
        act_h, noise_h = hidden_site(self.mode)
        act_v, noise_v = visible_site(self.mode)
        fe = d.free_energy(Vd, rows, lo)
        h = d.half_step("vh", Vd, rows, lo, act_h, noise_h, self.seed, base + 0, step)["sample"]
        v1 = d.half_step("hv", h, rows, 0, act_v, noise_v, self.seed, base + 1, step)["sample"]
        fe_p = d.free_energy(v1, rows, 0)
        return (fe - fe_p).abs().mean().reshape(1)

    def _labelled(self, V, y):
        """The training matrix of a label RBM as a DeviceMatrix [N, n_vis]: V [N, n_pix] joined with the one-hot block of the
        integer labels y, or (y None) V [N, n_vis] itself, whose block must be one-hot -- that is checked."""
        n_cols = V.cols if isinstance(V, DeviceMatrix) else V.shape[1]
        self._ensure_built(n_cols + (self.n_labels if y is not None else 0))
        Vd, _ = self._as_device(V)
        d, n_pix = self._dev, self._n_pix()
        if y is not None:
            if Vd.cols != n_pix:
                raise ValueError("V has %d columns; with y it holds the %d pixels alone" % (Vd.cols, n_pix))
            return self._with_label(Vd, y)
        if Vd.cols != d.n_vis:
            raise ValueError("V has %d columns, the label RBM has %d visible units (%d pixels + %d labels): pass y, or a joined matrix"
                             % (Vd.cols, d.n_vis, n_pix, self.n_labels))
        if Vd.rows:
            blk = Vd.t[:Vd.rows, n_pix:d.n_vis]
            if not bool((((blk == 0) | (blk == 1)).all() & (blk.sum(dim=1) == 1).all()).item()):
                raise ValueError("the last %d columns of V must be a one-hot label block (see RBM.join)" % self.n_labels)
        return Vd

    def fit(self, V, verbose=1, y=None):
        """Train the RBM on V [N, n_vis] by CD-k (rbm.py:100-234).

        y (label RBM only): integer labels in [0, n_labels), joined to V [N, n_pix] as the one-hot label block; without y, V must
        be n_vis wide and carry that block itself.  A label RBM trains on one GPU.

        V: numpy array, torch tensor (host or device) -- uploaded once and kept resident.
        verbose: 1 prints the epoch counter and the per-step score as the reference does
                 (rbm.py:114-115, :234); 0 prints nothing and skips the three score passes.
        Returns None.
        """
        V = _unwrap(V)
        if y is not None and not self.n_labels:
            raise ValueError("y needs a label RBM (n_labels > 0)")
        if self.n_labels:
            if dp.world()[1] > 1:
                raise ValueError("a label RBM has no data-parallel fit: train it on one GPU")
            V = self._labelled(V, y)
        n_cols = V.cols if isinstance(V, DeviceMatrix) else V.shape[1]
        self._ensure_built(n_cols)
        Vd, _ = self._as_device(V)
        if Vd.cols != self._dev.n_vis:
            raise ValueError("V has %d columns, the RBM has %d visible units" % (Vd.cols, self._dev.n_vis))
        bs = int(self.hps["batch_size"])
        lr = float(self.hps["lr"])
        n = Vd.rows
        num_step = n // bs if n % bs == 0 else n // bs + 1                     # rbm.py:110-111
        rank, world = dp.world()
        d = self._dev
        self.last_scores = []
        self._data_real = self.compute_dtype == "auto" and d.v_pieces(Vd) != 1   # ('auto' asks once what the data is)
        if self.persistent and self._v_chain is None:
            # fantasy particles start at the first batch of the data
            self._v_chain = DeviceMatrix.zeros(bs, d.n_vis, d.device)
            first = min(bs, n)
            self._v_chain.t[:first].copy_(Vd.t[:first])
        if self.persistent and (self._v_chain.rows != bs or self._v_chain.cols != d.n_vis):
            # every step reads and rewrites `rows` rows of the chain in place: a chain kept from a fit with another batch
            # size (or loaded from such a checkpoint) would be read past its end
            raise ValueError("the persistent chain has shape (%d, %d); hps['batch_size'] = %d and %d visible units need (%d, %d) -- "
                             "set rbm._v_chain = None to restart the chain from the data"
                             % (self._v_chain.rows, self._v_chain.cols, bs, d.n_vis, bs, d.n_vis))
        if self.objective != "generative":
            return self._fit_disc(Vd, n, bs, lr, num_step, verbose)

        # x3: the bf16 planes of every window of rows this fit walks are made once, here (the data is the same every
        # epoch); the fallback -- not enough HBM -- is the per-step conversion inside the library
        planes = None
        if self._compute() == "x3" and n > 0:
            windows = []
            for i in range(num_step):
                lo, rows = i * bs, min((i + 1) * bs, n) - i * bs
                if world > 1:
                    s_lo, s_hi = self._shard(rows, rank, world)
                    lo, rows = lo + s_lo, s_hi - s_lo
                windows.append((lo, rows))
            planes = d.make_planes(Vd, windows, self.mode, self._v_chain if self.persistent else None)
        self._planes = planes
        # quiet single-GPU fused training (fp32 MFMA or x3): the whole batch loop of an epoch is one library call
        whole_epochs = (verbose != 1 and world == 1 and self.update_mode == "fused"
                        and self._compute() in ("fp32", "x3", "small"))
        # ... and with the per-step score (the reference's default), for the one-launch small path
        scored_epochs = (verbose == 1 and world == 1 and self.update_mode == "fused" and self._compute() == "small" and bs <= 512)
        def print_score(score, label):
            self.last_scores.append(score)
            print("\n{0:d}/{1:d}, score: {2:f}".format(label[0], label[1], score))   # rbm.py:234
        ring = _ScoreRing(d.device, print_score) if verbose == 1 else None
        for epoch in range(int(self.hps["epochs"])):                              # rbm.py:113
            if verbose == 1:
                print(epoch + 1, "/", self.hps["epochs"], " epochs", end="\r")   # rbm.py:115
            # (the keyword is passed only when one of the two terms is set: the default path makes the plain calls, and engine
            # doubles without the keyword keep working)
            self._mom_kw = {"momentum": (self.momentum_at(self._epochs_done), self.weight_decay)} if self._has_momentum() else {}
            self._epochs_done += 1
            if whole_epochs:
                self._update_count += d.cd_epoch(Vd, n, bs, lr, self.seed, self._update_count, k=self.cd_k,
                                                 mode=self.mode, v_chain=self._v_chain if self.persistent else None,
                                                 compute=self._compute(), planes=planes, **self._mom_kw, **self._label_kw())
                continue
            if scored_epochs:
                # small RBMs with the reference's default verbose = 1: the epoch's updates AND scores are queued by one library
                # call (two launches per step); the scores land in pinned host memory, and the lines are printed, in order, as they do
                steps, scores = d.cd_epoch_small_scored(Vd, n, bs, lr, self.seed, self._update_count, self.mode, CHAIN_SCORE)
                self._update_count += steps
                flags = scores.numpy()
                for i in range(steps):
                    spins = 0
                    while flags[i, 1] != 1.0:
                        spins += 1
                        if spins > 2000:
                            time.sleep(50e-6)
                        if spins > 400000:     # (~20 s: the device never wrote it -- a skipped launch; the status word says why)
                            d.check_status()
                            raise _lib.KurbmError("the score of step %d never arrived" % (i + 1))
                    print_score(float(flags[i, 0]), (i + 1, num_step))
                continue
            for i in range(num_step):                                            # rbm.py:163
                lo, hi = i * bs, min((i + 1) * bs, n)                            # rbm.py:211 / :218
                rows = hi - lo
                step = self._update_count
                if world == 1:
                    self._update_local(Vd, lo, rows, lr, step)
                else:
                    self._update_data_parallel(Vd, lo, rows, lr, step, rank, world)
                self._update_count += 1
                if verbose == 1:
                    # (the line of step i is printed when its score has landed: at most one step late, never out of order)
                    ring.push(self._score(Vd, lo, rows, step), (i + 1, num_step))
            if ring is not None:
                ring.flush()                                                     # an epoch's lines end with the epoch
        self._planes = None
        d.check_status()                  # fit() ends with one status read: no later call trains on from a skipped update
        return None

    def _fit_disc(self, Vd, n, bs, lr, num_step, verbose):
        """The batch loop of fit() for objective 'discriminative' / 'hybrid' (kurbm_disc_step; one GPU, as every label RBM): the
        epoch call with verbose = 0; with verbose = 1 a step per batch, its score the batch's mean nll = -log p(y | v) BEFORE the
        update, printed in the reference's format through the score ring.  _update_count advances by one per batch; it is the
        `step` of the generative chain of a hybrid update, and a discriminative one draws nothing."""
        d = self._dev
        if self.update_mode != "fused":
            raise ValueError("objective %r makes one fused update per batch: update_mode='fused'" % self.objective)
        gw = self.gen_weight if self.objective == "hybrid" else 0.0
        kw = dict(gen_weight=gw, seed=self.seed, k=self.cd_k, v_chain=self._v_chain if (self.persistent and gw > 0) else None)

        def print_score(score, label):
            self.last_scores.append(score)
            print("\n{0:d}/{1:d}, score: {2:f}".format(label[0], label[1], score))   # rbm.py:234
        ring = _ScoreRing(d.device, print_score) if verbose == 1 else None
        for epoch in range(int(self.hps["epochs"])):
            if verbose == 1:
                print(epoch + 1, "/", self.hps["epochs"], " epochs", end="\r")
            mom = {"momentum": (self.momentum_at(self._epochs_done), self.weight_decay)} if self._has_momentum() else {}
            self._epochs_done += 1
            if verbose != 1:
                self._update_count += d.disc_epoch(Vd, n, bs, lr, self.n_labels, step0=self._update_count, **kw, **mom)
                continue
            for i in range(num_step):
                lo, hi = i * bs, min((i + 1) * bs, n)
                nll = d.disc_step(Vd, hi - lo, lo, lr, self.n_labels, step=self._update_count, want_nll=True, **kw, **mom)
                self._update_count += 1
                ring.push(nll, (i + 1, num_step))
            ring.flush()
        d.check_status()
        return None

    def class_log_likelihood(self, V, y):
        """mean log p(y | v) over the rows of V [N, n_pix] (or [N, n_vis]: the block is ignored) for integer labels y [N], on the
        host in float64 from class_logits: logit_y - logsumexp(logit), which stays finite where p(y | v) underflows."""
        logits, _, _ = self._class_logits(V)
        lg = logits.to_numpy().astype(np.float64)
        y = self._labels(y, lg.shape[0])
        if lg.shape[0] == 0:
            return float("nan")
        m = lg.max(axis=1)
        lse = m + np.log(np.exp(lg - m[:, None]).sum(axis=1))
        return float((lg[np.arange(lg.shape[0]), y] - lse).mean())

    def momentum_at(self, epoch):
        """mu of epoch `epoch` (0-based, counted over every fit() of this object): a schedule's last value holds from its end on."""
        m = self.momentum
        return m[min(int(epoch), len(m) - 1)] if isinstance(m, list) else m

    def _label_kw(self):
        """The `n_labels=` keyword of the engine's step calls; empty for an ordinary RBM, whose calls stay as they were."""
        return {"n_labels": self.n_labels} if self.n_labels else {}

    def _has_momentum(self):
        m = self.momentum
        return self.weight_decay != 0.0 or (any(x != 0.0 for x in m) if isinstance(m, list) else m != 0.0)

    def _compute(self):
        """The compute path of this fit.  'auto' reads tools/small_crossover.py's tables (784 visible units, one MI355X;
        profiles/r04_e_compute_path_crossover.txt):
        * the one-launch step (CD-1 from the data, one GPU) up to batch 128 with up to 1024 hidden units, batch 256 with up to 512 and
          batch 384 with up to 256, batch 512 with up to 128 -- 21-56 us per step where the multi-launch paths take 55-110;
        * 0/1 data in Bernoulli mode: x3 at every other size (it beats the fp32-MFMA launches from batch 64 on);
        * real-valued data or Gaussian visibles (three pieces per value, seven launches): x3 from rows x n_vis x n_hid >= 6e8 on
          (batch 1024 at 784 x 1024, 1536 at 784 x 512), the fp32-MFMA kernels below.
        The five-launch 'fp32' path whatever was asked once n_labels > 0 -- the same rule as momentum on 'small': the label site
        exists on that path only (the x3 path for label RBMs is a named follow-up)."""
        c = self.compute_dtype
        if self.n_labels:
            return "fp32"
        small_ok = self.cd_k == 1 and not self.persistent and dp.world()[1] == 1 and not self._has_momentum()
        if c == "auto":
            b, h = int(self.hps["batch_size"]), int(self.output_dim)
            if small_ok and ((b <= 128 and h <= 1024) or (b <= 256 and h <= 512) or (b <= 384 and h <= 256) or (b <= 512 and h <= 128)):
                return "small"
            real = self.mode == MODE_VISIBLE_GAUSSIAN or getattr(self, "_data_real", False)
            n_vis = self._dev.n_vis if self._dev is not None else 784
            return "x3" if (not real or float(b) * n_vis * h >= 6e8) else "fp32"
        if c == "small" and not small_ok:
            return "fp32"     # the one-launch step is CD-1 from the data on one GPU, bare rule; everything else runs the five-launch path
        return c

    def _update_local(self, Vd, lo, rows, lr, step):
        d = self._dev
        if self.update_mode == "fused":
            d.cd_step(Vd, rows, lo, lr, self.seed, step, k=self.cd_k, mode=self.mode, chain=CHAIN_W,
                      v_chain=self._v_chain if self.persistent else None, compute=self._compute(), planes=self._planes,
                      **self._mom_kw, **self._label_kw())
        else:
            # the reference's three K.function calls: each its own chain, each seeing the variables
            # the previous call already updated (rbm.py:214-216)
            for chain, which in ((CHAIN_W, _lib.WHICH_W), (CHAIN_BH, _lib.WHICH_BH), (CHAIN_BV, _lib.WHICH_BV)):
                d.cd_step(Vd, rows, lo, lr, self.seed, step, k=1, mode=self.mode, chain=chain, which=which,
                          compute=self._compute(), planes=self._planes, **self._mom_kw, **self._label_kw())

    def _update_data_parallel(self, Vd, lo, rows, lr, step, rank, world):
        """Each rank: the chain on its rows of the batch -> packed sums -> sum all-reduce (RCCL, inside libkurbm.so) ->
        the identical update on every replica.  Philox counters use the row's index in the global batch (row0)."""
        if self.update_mode != "fused":
            raise ValueError("data-parallel training supports update_mode='fused' only")
        d = self._dev
        s_lo, s_hi = self._shard(rows, rank, world)
        d.cd_step_dp(dp.get_exchange(d.device, d.n_vis, d.n_hid), Vd, s_hi - s_lo, lo + s_lo, lr, self.seed, step, k=self.cd_k, mode=self.mode,
                     chain=CHAIN_W, row0=s_lo, v_chain=self._v_chain if self.persistent else None, v_chain_row=s_lo,
                     compute=self._compute(), planes=self._planes, **self._mom_kw)

    def full_chain(self):
        """The persistent chain as ONE host array [batch_size, n_vis], or None.  Under data parallelism rank r advances
        only its own rows of the chain (`_shard`); every other row it holds is stale.  This call is then COLLECTIVE: each
        rank contributes its rows, zeros elsewhere, to a sum all-reduce on the library's communicator, and every rank
        returns the assembled chain."""
        if self._v_chain is None:
            return None
        rank, world = dp.world()
        if world == 1:
            return self._v_chain.to_numpy()
        lo, hi = self._shard(self._v_chain.rows, rank, world)
        with device_guard(self._dev.device):
            own = torch.zeros_like(self._v_chain.t)
            own[lo:hi].copy_(self._v_chain.t[lo:hi])
            dp.get_exchange(self._dev.device, self._dev.n_vis, self._dev.n_hid).allreduce_sum_(own.view(-1))
            return own[: self._v_chain.rows, : self._v_chain.cols].contiguous().cpu().numpy()

    def _shard(self, rows, rank, world):
        """This rank's rows [lo, hi) of a batch of `rows` rows (persistent chains: fixed ownership of the chain's rows,
        whatever the batch's row count)."""
        return dp.shard_rows(rows, world, rank, of=int(self.hps["batch_size"]) if self.persistent else None)

    # ------------------------------------------------------------------ config ----------
    def get_config(self):
        """hps, output_dim, name as in rbm.py:236-242, plus `mode` (dropped by the reference) and the
        extension knobs, so that RBM(**config) rebuilds the same layer."""
        config = {"hps": self.hps, "output_dim": self.output_dim, "name": self.name, "mode": self.mode,
                  "seed": self.seed, "update_mode": self.update_mode, "cd_k": self.cd_k,
                  "persistent": self.persistent, "compute_dtype": self.compute_dtype,
                  "momentum": list(self.momentum) if isinstance(self.momentum, list) else self.momentum,
                  "weight_decay": self.weight_decay, "n_labels": self.n_labels,
                  "objective": self.objective, "gen_weight": self.gen_weight}
        return dict(list(self._kwargs.items()) + list(config.items()))


__all__ = ["RBM", "MODE_VISIBLE_BERNOULLI", "MODE_VISIBLE_GAUSSIAN", "MODE_COMPLEX"]
