"""Deep belief network: an ordered stack of RBMs trained greedily, layer by layer.

Host-side mirror of the reference ``ku.ebm.DBN`` (reference ku/ebm/dbn.py:11-95) with the
repairs listed in SURVEY.md 8(a): ``self.rbm_layer`` -> the argument / loop variable
(dbn.py:25, :28, :54-55, :94), ``rbm_layers`` -> ``_rbm_layers`` (dbn.py:27), and the empty
``range(len(layers), -1)`` of ``inv_transform`` -> a reverse walk (dbn.py:92).  All compute is in
the RBM layers; between layers the data stays on the device.
"""
from .engine import DeviceMatrix
from .rbm import _unwrap


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

    def sample(self, n_samples, burn_in=1000, thin=100, n_chains=None, init=None, return_prob=False, seed=None, label=None):
        """n_samples "dreams" of the network (extension), [n_samples, n_vis of the first layer]: a Gibbs run in the TOP RBM
        (RBM.sample: burn_in, thin, n_chains, seed as there), then one ancestral pass down through inv_transform of the lower
        layers, in the order of DBN.inv_transform.  init [n_chains, n_vis of the first layer] starts the top chains from its
        sampled representation (layer.transform up to the top RBM's input).  return_prob: the bottom layer's visible_probs of the
        last hidden states instead of its sample.  A host array, or where init came from.
        label (a label RBM on top): the class, or one per chain, whose one-hot block the top chains start from and keep; only the
        pixel part of the top RBM's states goes down."""
        layers = self._layers()
        if not all(layer.built for layer in layers):
            raise ValueError("sample needs built RBM layers")
        kind, top_init = "numpy", None
        if init is not None:
            top_init, kind = self._to_device(layers[0], init)
            for rbm_layer in layers[:-1]:
                top_init = rbm_layer.transform(top_init)
        n_samples = int(n_samples)
        H_p, _, _ = layers[-1]._sample(n_samples, n_chains, burn_in, thin, top_init, None, False, seed, label)
        if self._top_labels() and len(layers) > 1:     # the label block stays up there: the layer below sees the pixel columns
            H_p = DeviceMatrix(H_p.t, H_p.rows, H_p.cols - self._top_labels(), H_p.ld)
        if H_p.rows != n_samples:                 # (kept, chain) order: the first n_samples rows
            H_p = DeviceMatrix(H_p.t, n_samples, H_p.cols, H_p.ld)
        if len(layers) == 1:
            if return_prob:
                raise ValueError("return_prob needs a layer below the top RBM (use RBM.sample(return_prob=True))")
            return layers[0]._ret(H_p, kind, False)
        for rbm_layer in reversed(layers[1:-1]):
            H_p = rbm_layer.inv_transform(H_p)
        H_p = layers[0].visible_probs(H_p) if return_prob else layers[0].inv_transform(H_p)
        return layers[0]._ret(H_p, kind, False)
