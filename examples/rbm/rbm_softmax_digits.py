#!/usr/bin/env python3
"""RBM features -> softmax digit classifier, on MI355X.

The caller on one side of the hot path: the shape of the reference's
examples/rbm/rbm_softmax_mnist.py -- a `MNISTClassifier(conf)` with `train()` / `test()`, an RBM trained
unsupervised by `rbm.fit(V)` (reference :83), whose STOCHASTIC hidden features `rbm(x)` (reference :58,
ku/ebm/rbm.py:80-86) feed a 10-way softmax layer trained with Adam (reference :61-72, :87-91), and
`test()` writing `solution.csv` (reference :123-127).

Data: Kaggle `train.csv` / `test.csv` in the working directory if present (reference :98, :131);
otherwise scikit-learn's bundled 8x8 digits, scaled to [0,1] and nearest-neighbour upsampled to
28x28 = 784 pixels (MNIST itself is not available offline).  The RBM runs on the HIP kernels; the
softmax head is a torch Linear layer on the same device (it is not part of the hot path).

`rbm_hps` of the JSON config also takes `momentum` (a number, or a list indexed by epoch whose last value holds:
[0.5, 0.5, 0.5, 0.5, 0.5, 0.9]) and `weight_decay` (on the scale of the batch SUMS that `lr` multiplies); both default to
0, the reference's bare update rule.  `objective` is what `fit` climbs: "generative" (the default: CD, as the reference trains)
is the only one for this example's plain RBM; "discriminative" and "hybrid" (with `gen_weight`) train a label RBM
(`n_labels`, `fit(V, y=labels)`) on log p(y | v), which then classifies by itself through `rbm.predict` -- README.md,
"Discriminative and hybrid training".

An optional top-level key `"fine_tune"` (absent by default: nothing changes) adds a second classifier after the run: a label RBM
(`n_labels = 10`) stacked on the trained RBM as a DBN, pretrained greedily on the RBM's mean-field features and then fine-tuned
end to end on log p(y | v) by `DBN.fine_tune` -- e.g. `{"top_hidden": 128, "top_hps": {"lr": 0.001, "epochs": 5, "batch_size": 128},
"epochs": 10, "lr": 0.0005, "momentum": 0.5, "weight_decay": 0.0}`.  Its held-out accuracy is printed before and after
fine-tuning.  README.md, "Fine-tuning a DBN".

An optional top-level key `"joint_model"` (absent by default: nothing changes) trains a label RBM (`n_labels = 10`, Bernoulli
visibles) generatively on `[pixels | one-hot label]` and uses it as the generative model it is: the mean `log p(v, y)` and
`log p(v)` of the held-out digits under an AIS estimate of log Z (`label="free"`), and a few joint samples `(v, y)` from Gibbs
chains whose label block is free -- e.g. `{"hidden": 128, "hps": {"lr": 0.001, "epochs": 10, "batch_size": 128}, "n_chains": 256,
"betas": 1000, "n_samples": 5, "burn_in": 500}`.  README.md, "Free label blocks".
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ku.ebm import DBN, RBM  # noqa: E402
from keras_unsupervised_amd.ebm import load_rbm, save_rbm  # noqa: E402


def load_digits_784():
    from sklearn.datasets import load_digits
    d = load_digits()
    img = (d.images / 16.0).astype(np.float32)                       # [n, 8, 8] in [0, 1]
    up = np.repeat(np.repeat(img, 4, axis=1), 4, axis=2)[:, 2:30, 2:30]   # 32x32 -> centre 28x28
    return up.reshape(len(up), 784), d.target.astype(np.int64)


class MNISTClassifier(object):
    """Digit classifier: RBM (unsupervised, CD) + softmax (supervised)."""

    MODEL_STEM = "digit_classification_model"
    IMAGE_SIZE = 784

    def __init__(self, conf, workdir="."):
        self.conf, self.workdir = conf, workdir
        self.hps, self.nn_arch = conf["hps"], conf["nn_arch"]
        self.device = torch.device("cuda", torch.cuda.current_device())
        stem = os.path.join(workdir, self.MODEL_STEM)
        if conf.get("model_loading"):
            self.rbm = load_rbm(stem + ".rbm")
            self.head = torch.nn.Linear(self.nn_arch["output_dim"], 10).to(self.device)
            self.head.load_state_dict(torch.load(stem + ".head.pt", map_location=self.device))
        else:
            self.rbm = RBM(conf["rbm_hps"], self.nn_arch["output_dim"], name="rbm",
                           mode=conf.get("rbm_mode", 1))            # reference default mode: Gaussian
            self.head = torch.nn.Linear(self.nn_arch["output_dim"], 10).to(self.device)

    # -- data -----------------------------------------------------------------------------
    def _load_training_data(self):
        path = os.path.join(self.workdir, "train.csv")
        if self.conf.get("data", "auto") != "digits" and os.path.exists(path):
            import pandas as pd
            df = pd.read_csv(path)
            return (df.iloc[:, 1:].values / 255.0).astype(np.float32), df.iloc[:, 0].values.astype(np.int64)
        V, y = load_digits_784()
        n = int(0.8 * len(V))
        return V[:n], y[:n]

    def _load_test_data(self):
        path = os.path.join(self.workdir, "test.csv")
        if self.conf.get("data", "auto") != "digits" and os.path.exists(path):
            import pandas as pd
            return (pd.read_csv(path).values / 255.0).astype(np.float32), None
        V, y = load_digits_784()
        n = int(0.8 * len(V))
        return V[n:], y[n:]

    # -- model ----------------------------------------------------------------------------
    def _features(self, Vt):
        """rbm(x): sampled hidden units, fresh draws on every call (the layer's forward pass)."""
        return self.rbm(Vt)

    def train(self, verbose=1):
        V, y = self._load_training_data()
        print("Train the RBM model.")
        self.rbm.fit(V, verbose=0)
        print("Train the NN model.")
        Vt = torch.from_numpy(V).to(self.device)
        yt = torch.from_numpy(y).to(self.device)
        opt = torch.optim.Adam(self.head.parameters(), lr=self.hps["lr"] * 10,
                               betas=(self.hps["beta_1"], self.hps["beta_2"]))
        bs = self.hps["batch_size"]
        for epoch in range(self.hps["epochs"]):
            tot = 0.0
            for lo in range(0, len(V), bs):
                x = self._features(Vt[lo:lo + bs].contiguous())
                loss = torch.nn.functional.cross_entropy(self.head(x), yt[lo:lo + bs])
                opt.zero_grad()
                loss.backward()
                opt.step()
                tot += float(loss.detach()) * len(x)
            if verbose:
                print("epoch %d/%d  loss %.4f" % (epoch + 1, self.hps["epochs"], tot / len(V)))
        print("Save the model.")
        stem = os.path.join(self.workdir, self.MODEL_STEM)
        save_rbm(self.rbm, stem + ".rbm")
        torch.save(self.head.state_dict(), stem + ".head.pt")

    def predict(self, V, n_draws=8):
        """Class probabilities, averaged over a few stochastic feature draws."""
        Vt = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).to(self.device)
        with torch.no_grad():
            p = sum(torch.softmax(self.head(self._features(Vt)), dim=1) for _ in range(n_draws)) / n_draws
        return p.cpu().numpy()

    def test(self):
        V, y = self._load_test_data()
        res = self.predict(V)
        with open(os.path.join(self.workdir, "solution.csv"), "w") as f:
            f.write("ImageId,Label\n")
            for i, v in enumerate(res):
                f.write(str(i + 1) + "," + str(int(np.argmax(v))) + "\n")
        acc = float((res.argmax(1) == y).mean()) if y is not None else None
        if acc is not None:
            print("held-out accuracy: %.4f" % acc)
        return acc


def fine_tune_demo(mc, ft):
    """The opt-in "fine_tune" key: a label RBM on top of mc.rbm, greedy pretraining of that top layer, then DBN.fine_tune."""
    V, y = mc._load_training_data()
    Vt, yt = mc._load_test_data()
    top_hps = ft.get("top_hps", mc.conf["rbm_hps"])
    top = RBM(top_hps, int(ft.get("top_hidden", 128)), name="top", mode=0, n_labels=10, seed=int(ft.get("seed", 11)))
    dbn = DBN()
    dbn.add_stack(mc.rbm)
    dbn.add_stack(top)
    print("Pretrain the label RBM on the RBM's mean-field features.")
    top.fit(mc.rbm.hidden_probs(V), y=y, verbose=0)
    acc = lambda: float((dbn.predict(Vt) == yt).mean()) if yt is not None else float("nan")
    ll0, acc0 = dbn.class_log_likelihood(V, y), acc()
    print("Fine-tune every layer on log p(y | v).")
    dbn.fine_tune(V, y, epochs=ft.get("epochs"), lr=ft.get("lr"), batch_size=ft.get("batch_size"), momentum=ft.get("momentum", 0.0),
                  weight_decay=ft.get("weight_decay", 0.0), verbose=0)
    ll1, acc1 = dbn.class_log_likelihood(V, y), acc()
    print("DBN: mean log p(y | v) on the training set %.4f -> %.4f, held-out accuracy %.4f -> %.4f" % (ll0, ll1, acc0, acc1))
    return acc0, acc1


def joint_model_demo(mc, jm):
    """The opt-in "joint_model" key: log p(v, y) and joint samples of a generatively trained label RBM (label="free")."""
    V, y = mc._load_training_data()
    Vt, yt = mc._load_test_data()
    rbm = RBM(jm.get("hps", mc.conf["rbm_hps"]), int(jm.get("hidden", 128)), name="joint", mode=0, n_labels=10, seed=int(jm.get("seed", 11)))
    print("Train a label RBM on [pixels | one-hot label].")
    rbm.fit(V, y=y, verbose=0)
    log_z = rbm.log_partition(n_chains=int(jm.get("n_chains", 256)), betas=int(jm.get("betas", 1000)), base_rates=rbm.join(V, y),
                              label="free")
    print("log Z = %.3f +- %.3f (AIS, %d chains)" % (log_z, rbm.last_ais["stderr"], rbm.last_ais["n_chains"]))
    if yt is not None:
        print("held-out mean log p(v, y) = %.3f, mean log p(v) = %.3f"
              % (rbm.log_likelihood(Vt, y=yt, log_z=log_z, label="free"), rbm.log_likelihood(Vt, log_z=log_z, label="free")))
    n = int(jm.get("n_samples", 5))
    S = rbm.sample(n, burn_in=int(jm.get("burn_in", 500)), label="free")
    for row in S:
        print("sampled class %d with %d of %d pixels on" % (int(row[-10:].argmax()), int(row[:-10].sum()), row.size - 10))
    return log_z


def main():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rbm_softmax_conf.json")) as f:
        conf = json.load(f)
    mc = MNISTClassifier(conf)
    ts = time.time()
    if conf["mode"] == "train":
        mc.train()
        mc.test()
    else:
        mc.test()
    if conf.get("fine_tune"):
        fine_tune_demo(mc, conf["fine_tune"])
    if conf.get("joint_model"):
        joint_model_demo(mc, conf["joint_model"])
    print("Elapsed time: {0:f}s".format(time.time() - ts))


if __name__ == "__main__":
    main()
