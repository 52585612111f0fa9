"""Deep belief network: an ordered stack of RBMs trained greedily, layer by layer.

Host-side mirror of the reference ``ku.ebm.DBN`` (reference ku/ebm/dbn.py:11-95) with the
repairs listed in SURVEY.md 8(a): ``self.rbm_layer`` -> the argument / loop variable
(dbn.py:25, :28, :54-55, :94), ``rbm_layers`` -> ``_rbm_layers`` (dbn.py:27), and the empty
``range(len(layers), -1)`` of ``inv_transform`` -> a reverse walk (dbn.py:92).  All compute is in
the RBM layers; between layers the data stays on the device.
"""
import torch

from . import dp
from .engine import DeviceMatrix, device_guard, hidden_site
from .rbm import _ScoreRing, _unwrap

WHICH_W_BH = 3      # a lower layer's apply: W and b_h (its db_v is zero; its visible bias and that velocity are left alone)


def _dims(layer):
    """(n_in, n_out) of a layer; n_in is None until the layer is built.  A label RBM (n_labels > 0) takes the layer below on
    its PIXEL units: its label block is not fed from below."""
    n_in = layer.input_shape[1] if getattr(layer, "input_shape", None) else None
    if n_in is not None:
        n_in -= getattr(layer, "n_labels", 0)
    out_shape = getattr(layer, "output_shape", None)
    n_out = out_shape[1] if out_shape else layer.output_dim
    return n_in, n_out


class DBN(object):
    """Deep belief network."""

    def add_stack(self, rbm_layer):
        """Append an RBM; its input width must equal the previous layer's output width
        (dbn.py:14-32).  An unbuilt layer has no input width yet and is checked when it is built
        by fit / transform."""
        if hasattr(self, "_rbm_layers"):
            if getattr(self._rbm_layers[-1], "n_labels", 0):
                raise ValueError("a label RBM is the top of a DBN: nothing stacks on its hidden layer here")
            n_in, _ = _dims(rbm_layer)
            _, prev_out = _dims(self._rbm_layers[-1])
            if n_in is not None and prev_out != n_in:
                raise ValueError("A previous RBM layer's output dimension must "
                                 "be equal to a next one's input dimension.")      # dbn.py:29-30
            self._rbm_layers.append(rbm_layer)
        else:
            self._rbm_layers = [rbm_layer]

    def _layers(self):
        if not hasattr(self, "_rbm_layers"):
            raise ValueError("Any rbm layer doesn't exist.")                       # dbn.py:47-48
        return self._rbm_layers

    @staticmethod
    def _to_device(layer, X):
        X = _unwrap(X)
        if isinstance(X, DeviceMatrix):
            return X, "device"
        layer._ensure_built(X.shape[1])
        return layer._as_device(X)

    def _top_labels(self):
        return getattr(self._layers()[-1], "n_labels", 0)

    def fit(self, V, verbose=1, y=None):
        """Greedy layer-wise training (dbn.py:34-55): fit layer l on V_p, then
        V_p <- layer.transform(V_p) -- the next layer sees SAMPLED hidden states.
        y (integer labels; needs a label RBM as the top layer): joined to the top layer's input as its one-hot block."""
        layers = self._layers()
        if (y is not None) != bool(self._top_labels()):
            raise ValueError("y goes with a label RBM (n_labels > 0) as the top layer, and such a top layer needs y")
        if len(layers) == 1 and y is not None:
            print("Train {0:s}.".format(str(layers[0].name)))
            layers[0].fit(V, verbose=verbose, y=y)
            return
        V_p, _ = self._to_device(layers[0], V)      # the reference's V.copy(): V itself is never written
        for rbm_layer in layers:
            print("Train {0:s}.".format(str(rbm_layer.name)))                      # dbn.py:53
            if rbm_layer is layers[-1] and y is not None:
                rbm_layer.fit(V_p, verbose=verbose, y=y)      # (its features are nobody's input: no transform behind it)
                break
            rbm_layer.fit(V_p, verbose=verbose)
            V_p = rbm_layer.transform(V_p)

    def predict_proba(self, V):
        """p(y | v) of a DBN whose top layer is a label RBM, mean-field: the hidden_probs of the lower layers, then the top layer's
        exact class posterior of those features.  [N, n_labels], where V came from."""
        return self._classify(V, "predict_proba")

    def predict(self, V):
        """argmax of predict_proba, integers [N]."""
        return self._classify(V, "predict")

    def _classify(self, V, what):
        layers = self._layers()
        if not self._top_labels():
            raise ValueError("%s needs a label RBM (n_labels > 0) as the top layer" % what)
        if len(layers) == 1:
            return getattr(layers[0], what)(V)
        V_p, kind = self._to_device(layers[0], V)
        for rbm_layer in layers[:-1]:
            V_p = rbm_layer.hidden_probs(V_p)
        out = getattr(layers[-1], what)(V_p)            # (a DeviceMatrix, or a device tensor of classes)
        if what == "predict":
            return out.cpu().numpy() if kind == "numpy" else (out if kind == "device" else out.to(kind))
        return layers[0]._ret(out, kind, False)

    def class_log_likelihood(self, V, y):
        """mean log p(y | v) over the rows of V for integer labels y [N]: predict_proba's path (the hidden_probs of the lower layers),
        then the top layer's class_log_likelihood of those features -- float64 on the host from the class logits."""
        layers = self._layers()
        if not self._top_labels():
            raise ValueError("class_log_likelihood needs a label RBM (n_labels > 0) as the top layer")
        if len(layers) == 1:
            return layers[0].class_log_likelihood(V, y)
        V_p, _ = self._to_device(layers[0], V)
        for rbm_layer in layers[:-1]:
            V_p = rbm_layer.hidden_probs(V_p)
        return layers[-1].class_log_likelihood(V_p, y)

    def fine_tune(self, V, y, epochs=None, lr=None, batch_size=None, momentum=0.0, weight_decay=0.0, verbose=1):
        """Fine-tune EVERY layer on sum log p(y | v) by backpropagation (extension; Hinton & Salakhutdinov 2006, Larochelle &
        Bengio 2008 section 6): the step after greedy pretraining (fit).  include/kurbm.h ("fine-tuning a DBN") states the model.

        The forward pass is predict_proba's -- the prob-only half steps of the lower layers, sigmoid or relu by their mode, no
        draw -- and the gradient is exact: the top label RBM's discriminative gradient, then act'(x) and two GEMMs per layer going
        down.  All on the fp32-MFMA launches; no random number is drawn, and two runs give the same bits.

        V [N, n_vis of the first layer], y integer labels [N].  epochs, lr, batch_size: default to the TOP layer's hps.  Batches are
        contiguous and unshuffled, remainder last.  Per batch: the forward launches, the top layer's backward call, the lower
        layers' from the top down, then every layer's params += lr * (its batch sums) -- all gradients at the weights the step
        started from, all queued on one stream with no host round trip inside an epoch.
        momentum (a float, or a sequence indexed by the epoch OF THIS CALL whose last value holds for later epochs) and
        weight_decay: RBM's rule, vel <- mu vel + lr (g - weight_decay W); W += vel (biases: no decay), through each layer's own
        velocity (the one its fit() uses: rbm._dev.set_velocity resets it).  A lower layer's visible bias is not a parameter of
        p(y | v) and is left alone.
        verbose = 1 prints each batch's mean -log p(y | v) BEFORE its update in fit()'s format (kept in self.last_scores).
        Every layer's update counter advances by the number of steps, so cached AIS results are discarded.  Returns None."""
        layers = self._layers()
        top, lower = layers[-1], layers[:-1]
        C = self._top_labels()
        if not C:
            raise ValueError("fine_tune needs a label RBM (n_labels > 0) as the top layer")
        if not all(layer.built for layer in layers):
            raise ValueError("fine_tune needs built RBM layers: pretrain the stack with fit(V, y=...) first")
        if dp.world()[1] > 1:
            raise ValueError("fine_tune has no data-parallel path: run it on one GPU")
        epochs = int(top.hps["epochs"] if epochs is None else epochs)
        lr = float(top.hps["lr"] if lr is None else lr)
        bs = int(top.hps["batch_size"] if batch_size is None else batch_size)
        if epochs < 0 or bs <= 0:
            raise ValueError("epochs must be >= 0 and batch_size positive")
        sched = [float(m) for m in momentum] if isinstance(momentum, (list, tuple)) else [float(momentum)]
        weight_decay = float(weight_decay)
        if not sched or any(not 0.0 <= m < 1.0 for m in sched):
            raise ValueError("momentum must be in [0, 1) (a number or a non-empty per-epoch sequence)")
        if not weight_decay >= 0.0:
            raise ValueError("weight_decay must be >= 0")
        with_mom = weight_decay != 0.0 or any(m != 0.0 for m in sched)
        Vd, _ = self._to_device(layers[0], V)
        n = Vd.rows
        if lower and Vd.cols != lower[0]._dev.n_vis:
            raise ValueError("V has %d columns, the first layer has %d visible units" % (Vd.cols, lower[0]._dev.n_vis))
        yh = top._labels(y, n)
        td, n_pix = top._dev, top._n_pix()
        acts = [hidden_site(layer.mode)[0] for layer in lower]
        with device_guard(td.device):
            if lower:
                onehot = torch.zeros((max(n, 1), C), dtype=torch.float32, device=td.device)
                if n:
                    onehot[torch.arange(n, device=td.device), torch.from_numpy(yh).to(td.device)] = 1.0
                # x_l, the lower layers' activations of a batch: the last one lives in the pixel columns of the top layer's batch plane
                plane = DeviceMatrix.zeros(bs, td.n_vis, td.device)
                xs = [DeviceMatrix.zeros(bs, layer._dev.n_hid, td.device) for layer in lower[:-1]] + [plane]
                es = [DeviceMatrix.zeros(bs, layer._dev.n_hid, td.device) for layer in lower]       # e_l = dL/dx_l, then delta_l
            else:
                plane = top._with_label(Vd, yh)       # a one-layer DBN: the step is RBM.fit(objective='discriminative')'s
        num_step = (n + bs - 1) // bs
        self.last_scores = []

        def print_score(score, label):
            self.last_scores.append(score)
            print("\n{0:d}/{1:d}, score: {2:f}".format(label[0], label[1], score))
        ring = _ScoreRing(td.device, print_score) if verbose == 1 else None
        for epoch in range(epochs):
            if verbose == 1:
                print(epoch + 1, "/", epochs, " epochs", end="\r")
            mom = {"momentum": (sched[min(epoch, len(sched) - 1)], weight_decay)} if with_mom else {}
            for i in range(num_step):
                lo, rows = i * bs, min((i + 1) * bs, n) - i * bs
                if lower:
                    x_in, x_row = Vd, lo
                    for layer, act, x in zip(lower, acts, xs):
                        layer._dev.probs_into(x_in, rows, x_row, act, x)
                        x_in, x_row = x, 0
                    with device_guard(td.device):
                        plane.t[:rows, n_pix:n_pix + C].copy_(onehot[lo:lo + rows])
                    deltas = [None] * len(lower)
                    d_top, nll = td.disc_backprop(plane, C, rows, 0, e_in=es[-1], want_nll=verbose == 1)
                    for l in range(len(lower) - 1, -1, -1):
                        deltas[l] = lower[l]._dev.backprop_layer(acts[l], Vd if l == 0 else xs[l - 1], xs[l], es[l], rows,
                                                                 lo if l == 0 else 0, e_in=es[l - 1] if l > 0 else None)
                    for layer, delta in zip(lower, deltas):
                        layer._dev.apply_delta(lr, which=WHICH_W_BH, delta=delta, **mom)
                else:
                    d_top, nll = td.disc_backprop(plane, C, rows, lo, want_nll=verbose == 1)
                td.apply_delta(lr, delta=d_top, **mom)
                for layer in layers:
                    layer._update_count += 1
                if ring is not None:
                    ring.push(nll, (i + 1, num_step))
            if ring is not None:
                ring.flush()
        td.check_status()
        return None

    def transform(self, V):
        """Chain of layer.transform (dbn.py:57-75)."""
        layers = self._layers()
        V_p, kind = self._to_device(layers[0], V)
        for rbm_layer in layers:
            V_p = rbm_layer.transform(V_p)
        return layers[0]._ret(V_p, kind, False)

    def inv_transform(self, H):
        """Reverse chain of layer.inv_transform (dbn.py:77-95, loop repaired)."""
        layers = self._layers()
        H_p, kind = self._to_device(layers[-1], H) if layers[-1].built else (None, None)
        if H_p is None:
            raise ValueError("inv_transform needs built RBM layers")
        for rbm_layer in reversed(layers):
            H_p = rbm_layer.inv_transform(H_p)
        return layers[0]._ret(H_p, kind, False)

    def transform_probs(self, V):
        """Chain of layer.hidden_probs: the deterministic (mean-field) features of V, no draw anywhere (extension)."""
        layers = self._layers()
        V_p, kind = self._to_device(layers[0], V)
        for rbm_layer in layers:
            V_p = rbm_layer.hidden_probs(V_p)
        return layers[0]._ret(V_p, kind, False)

    def sample(self, n_samples, burn_in=1000, thin=100, n_chains=None, init=None, return_prob=False, seed=None, label=None,
               return_labels=False):
        """n_samples "dreams" of the network (extension), [n_samples, n_vis of the first layer]: a Gibbs run in the TOP RBM
        (RBM.sample: burn_in, thin, n_chains, seed as there), then one ancestral pass down through inv_transform of the lower
        layers, in the order of DBN.inv_transform.  init [n_chains, n_vis of the first layer] starts the top chains from its
        sampled representation (layer.transform up to the top RBM's input).  return_prob: the bottom layer's visible_probs of the
        last hidden states instead of its sample.  A host array, or where init came from.
        label (a label RBM on top): the class, or one per chain, whose one-hot block the top chains start from and keep; only the
        pixel part of the top RBM's states goes down.  label='free': the top chains sample the block too (RBM.sample).
        return_labels (a label RBM on top): additionally the class of each sample's top state, integers [n_samples] -- the sampled
        class with label='free', the given one otherwise -- as (samples, labels)."""
        layers = self._layers()
        if return_labels and not self._top_labels():
            raise ValueError("return_labels needs a label RBM on top")
        if not all(layer.built for layer in layers):
            raise ValueError("sample needs built RBM layers")
        kind, top_init = "numpy", None
        if init is not None:
            top_init, kind = self._to_device(layers[0], init)
            for rbm_layer in layers[:-1]:
                top_init = rbm_layer.transform(top_init)
        n_samples = int(n_samples)
        H_p, _, _ = layers[-1]._sample(n_samples, n_chains, burn_in, thin, top_init, None, False, seed, label)
        classes = None
        if return_labels:
            classes = H_p.view()[:n_samples, H_p.cols - self._top_labels():].argmax(dim=1)
            classes = classes.cpu().numpy() if kind == "numpy" else (classes if kind == "device" else classes.to(kind))
        if classes is not None:
            done = lambda out: (out, classes)
        else:
            done = lambda out: out
        if self._top_labels() and len(layers) > 1:     # the label block stays up there: the layer below sees the pixel columns
            H_p = DeviceMatrix(H_p.t, H_p.rows, H_p.cols - self._top_labels(), H_p.ld)
        if H_p.rows != n_samples:                 # (kept, chain) order: the first n_samples rows
            H_p = DeviceMatrix(H_p.t, n_samples, H_p.cols, H_p.ld)
        if len(layers) == 1:
            if return_prob:
                raise ValueError("return_prob needs a layer below the top RBM (use RBM.sample(return_prob=True))")
            return done(layers[0]._ret(H_p, kind, False))
        for rbm_layer in reversed(layers[1:-1]):
            H_p = rbm_layer.inv_transform(H_p)
        H_p = layers[0].visible_probs(H_p) if return_prob else layers[0].inv_transform(H_p)
        return done(layers[0]._ret(H_p, kind, False))
