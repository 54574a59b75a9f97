"""The MNIST label classifier that generated-label accuracy is scored with, trained and evaluated on the engine's own kernels.

The reference scores its MNIST samples with a frozen graph, mnist/mnist_dcnn/graph_optimized.pb, which the checkout does not hold.
What mnist/utils.py:276-298 shows of it is its interface: an input ``x``, a dropout keep-probability placeholder (fed 1.0) and an
output ``pred_class`` -- the interface of the "deep MNIST" convnet, rebuilt here WITHOUT its weights:

  x [n,28,28,1] in [0, 1] -> conv 5x5 SAME (1 -> 32) + bias -> relu -> max pool 2x2 -> [n,14,14,32]
                          -> conv 5x5 SAME (32 -> 64) + bias -> relu -> max pool 2x2 -> [n,7,7,64] -> reshape [n,3136] (NHWC order)
                          -> dense 3136 -> 1024 + bias, relu (the FEATURES) -> dropout(keep_prob) -> dense 1024 -> K -> logits

fp32 activations, single GPU.  The convolutions and dense layers are the fp32 gather GEMM, relu + max pool and dropout are
rcgan_relu_maxpool2_* / rcgan_dropout_* (csrc/classifier.hip), the loss is the sparse softmax cross-entropy (plain or forward-corrected
for noisy labels) and the optimiser the captured TF-form Adam.  ``MnistLabelClassifier(asset).predict`` is a ``predict_fn`` for
``eval_mnist.generated_label_accuracy``.  What the trainer shares with the CIFAR one is ``label_trainer.LabelTrainer``."""
import numpy as np
import torch

from . import _lib as L
from . import ops as O
from .label_trainer import LabelTrainer
from .runtime import Context, check_f32_matmul_precision

FEATURE_DIM = 1024
FLAT = 7 * 7 * 64
NAMES = ("conv1|w", "conv1|b", "conv2|w", "conv2|b", "fc1|w", "fc1|b", "fc2|w", "fc2|b")


def variable_shapes(n_classes=10):
    return [("conv1|w", (5, 5, 1, 32)), ("conv1|b", (32,)), ("conv2|w", (5, 5, 32, 64)), ("conv2|b", (64,)),
            ("fc1|w", (FLAT, FEATURE_DIM)), ("fc1|b", (FEATURE_DIM,)), ("fc2|w", (FEATURE_DIM, int(n_classes))), ("fc2|b", (int(n_classes),))]


def _truncated_normal(rs, shape, std):
    """tf.truncated_normal: values beyond two standard deviations are drawn again."""
    a = rs.randn(*shape)
    bad = np.abs(a) > 2.0
    while bad.any():
        a[bad] = rs.randn(int(bad.sum()))
        bad = np.abs(a) > 2.0
    return (std * a).astype(np.float32)


def create_mnist_classifier_variables(seed, n_classes=10):
    """[(name, shape, init)] of the eight arrays of the weight asset: weights truncated normal (std 0.1, re-drawn beyond two standard
    deviations), biases 0.1 -- the tutorial's weight_variable / bias_variable -- from numpy.random.RandomState(seed)."""
    if not 2 <= int(n_classes) <= L.MAX_CLASSES:
        raise ValueError("n_classes %r: 2..%d" % (n_classes, L.MAX_CLASSES))
    rs = np.random.RandomState(seed)
    return [(n, s, _truncated_normal(rs, s, 0.1) if n.endswith("|w") else np.full(s, 0.1, np.float32)) for n, s in variable_shapes(n_classes)]


def mnist_classifier_logits(ctx, w, x, keep_prob=None, rng=None, features=False):
    """The forward pass, written once: x [n,28,28,1] fp32 device tensor in [0, 1] (the sampler's range, which the reference feeds to
    ``x`` unchanged), w = {name: device tensor} under the asset's names ('/'-separated) -> logits [n,K].  keep_prob: None evaluates
    (no dropout: the reference feeds 1.0), a number in (0, 1] drops features with the device stream rng = (seed, state).  Recorded on
    the tape when ctx.recording is on and the weights require gradients.  features: also return the [n,1024] feature tensor."""
    n = x.shape[0]
    if tuple(x.shape[1:]) != (28, 28, 1):
        raise ValueError("expected [n,28,28,1] images, got %s" % (tuple(x.shape),))
    h = O.relu_maxpool2(ctx, O.conv2d(ctx, x, O.Weight(ctx, w["conv1/w"]), w["conv1/b"], 5))
    h = O.relu_maxpool2(ctx, O.conv2d(ctx, h, O.Weight(ctx, w["conv2/w"]), w["conv2/b"], 5))
    feat = O.act(ctx, O.linear(ctx, O.reshape(ctx, h, (n, FLAT)), O.Weight(ctx, w["fc1/w"]), w["fc1/b"]), L.ACT_RELU)
    t = feat
    if keep_prob is not None:
        if rng is None:
            raise ValueError("dropout needs rng = (seed, device stream state)")
        t = O.dropout(ctx, feat, keep_prob, rng[0], rng[1])
    logits = O.linear(ctx, t, O.Weight(ctx, w["fc2/w"]), w["fc2/b"])
    return (logits, feat) if features else logits


def check_images(images):
    """float [n,28,28,1] (or [n,784] rows) in [0, 1] -> contiguous float32 [n,28,28,1]."""
    x = np.ascontiguousarray(np.asarray(images, np.float32))
    if x.ndim == 2 and x.shape[1] == 784:
        x = x.reshape(-1, 28, 28, 1)
    if x.ndim != 4 or x.shape[1:] != (28, 28, 1):
        raise ValueError("expected [n,28,28,1] images, got %s" % (x.shape,))
    return x


def _forward_chunks(ctx, w, images, batch, fn):
    """fn(logits, features, lo, n) over the images ``batch`` at a time, recording off.  No sample's output depends on what else is in its batch
    (no batch norm), only -- in the last bits -- on the batch SIZE, which picks the GEMMs' summation order."""
    x = check_images(images)
    rec, ctx.recording = ctx.recording, False
    try:
        for lo in range(0, len(x), batch):
            ctx.new_step()
            part = x[lo:lo + batch]
            logits, feat = mnist_classifier_logits(ctx, w, ctx.upload(part, L.F32), features=True)
            fn(logits, feat, lo, len(part))
    finally:
        ctx.recording = rec


def _softmax(ctx, w, images, batch):
    out = []
    _forward_chunks(ctx, w, images, batch, lambda lg, ft, lo, n: out.append(ctx.download(O.softmax_rows(ctx, lg)).copy()))
    return np.concatenate(out, axis=0) if out else np.zeros((0, w["fc2/w"].shape[1]), np.float32)


class MnistClassifierTrainer(LabelTrainer):
    SLABS = (("m", "m"), ("v", "v"))
    _check_images = staticmethod(check_images)

    def __init__(self, n_classes=10, batch_size=128, keep_prob=0.5, beta1=0.9, beta2=0.999, eps=1e-8, device=0, seed=0, use_graphs=True,
                 variables=None, f32_matmul_precision="highest", confusion_matrix=None):
        """confusion_matrix: None trains on the labels as they are (sparse softmax cross-entropy).  A [K,K] row-stochastic matrix
        C[clean, noisy] declares the labels NOISY: the step then uses the forward-corrected loss -log((softmax(z) . C)[label]) (Patrini
        et al. 2017) and ``recover_labels`` becomes available -- the calls LabelClassifierTrainer makes."""
        check_f32_matmul_precision(f32_matmul_precision, "f32")
        if not 0.0 < float(keep_prob) <= 1.0:
            raise ValueError("keep_prob %r: (0, 1]" % (keep_prob,))
        specs = variables if variables is not None else create_mnist_classifier_variables(seed, n_classes)
        want = variable_shapes(n_classes)
        if [(n, tuple(s)) for n, s, _ in specs] != want:
            raise ValueError("variables %s, expected %s" % ([(n, tuple(s)) for n, s, _ in specs], want))
        self.keep_prob, self.beta1, self.beta2, self.eps = float(keep_prob), float(beta1), float(beta2), float(eps)
        self.seed = int(seed)
        # activations of a step at batch 128: ~30 MB with their gradients; evaluation at batch 1000: ~150 MB
        super().__init__(specs, n_classes, batch_size, self.seed, use_graphs, f32_matmul_precision, confusion_matrix, device, 1 << 30)

    def _make_buffers(self):
        ctx, B = self.ctx, self.B
        self.x = ctx.persistent((B, 28, 28, 1), L.F32, fill=0.0)
        self.draws = ctx.persistent((2 * B,), "i32", fill=0)         # [index (B) | labels (B)]: one upload per step
        self.index, self.labels = self.draws.rows(0, B), self.draws.rows(B, 2 * B)
        with torch.cuda.stream(ctx.stream):
            self.rng_state = torch.zeros(2, dtype=torch.int64, device=ctx.device)      # the dropout stream's offset, in quads
        self.dropout_seed = self.seed * 1000003 + 900007

    # ------------------------------------------------------------------------------------ data
    def load_data(self, images, labels):
        """The training set onto the device as fp32 rows of 784 in [0, 1]: images [N,28,28,1] or [N,784], in [0, 1] (the scaling
        data_mnist.corrupt / load_mnist hand to the GAN) or raw pixel values 0..255, which are divided by 255."""
        img = np.asarray(images, np.float32).reshape(len(labels), 784)
        lab = np.ascontiguousarray(np.asarray(labels).astype(np.int32))
        if not np.isfinite(img).all() or img.min() < 0:
            raise ValueError("images hold negative or non-finite values")
        if img.max() > 1.0:
            if img.max() > 255.0:
                raise ValueError("images outside [0, 1] and [0, 255]")
            img = img / np.float32(255.0)
        self._install_data(np.ascontiguousarray(img, np.float32), lab, labels_on_device=False)

    # ------------------------------------------------------------------------------------ step
    def _body(self):
        ctx, B = self.ctx, self.B
        ctx.new_step()
        self.P.zero_grad()
        ctx.check(ctx.lib.rcgan_gather_rows(ctx.h, B, 784, self.images.data_ptr(), self.index.ptr, self.x.ptr))
        self._loss(mnist_classifier_logits(ctx, self.w, self.x, keep_prob=self.keep_prob, rng=(self.dropout_seed, self.rng_state)))
        ctx.backward()
        self.P.adam_captured(self.beta1, self.beta2, self.eps)

    def step(self, lr, index=None):
        """One training step on the samples ``index`` [B] of the loaded set (drawn from the trainer's own numpy stream when not given).
        The dropout mask comes from the device stream (dropout_seed, rng_state), eager or replayed."""
        index = self._step_index(index)
        if index.shape != (self.B,):
            raise ValueError("index %s for batch size %d" % (index.shape, self.B))
        self._check_index_range(index)
        self.ctx.upload(np.concatenate([index, self.labels_all[index]]), out=self.draws)
        self.P.set_hyper_device(lr, self.steps + 1)
        self._run_step()

    def rng_offset(self):
        """The dropout stream's offset (quads drawn so far)."""
        with torch.cuda.stream(self.ctx.stream):
            v = self.rng_state.cpu()
        self.ctx.sync()
        return int(v[0])

    # ------------------------------------------------------------------------------------ evaluation
    def _forward_chunks(self, images, batch, fn):
        _forward_chunks(self.ctx, self.w, images, batch, lambda logits, feat, lo, n: fn(logits, lo, n))

    def evaluate(self, images, labels, batch=1000):
        """(accuracy, softmax [n,K]) on float [n,28,28,1] images in [0, 1], ``batch`` at a time, no dropout: the launches of
        MnistLabelClassifier.softmax."""
        p = _softmax(self.ctx, self.w, images, batch)
        return float((np.argmax(p, axis=1) == np.asarray(labels).reshape(-1)).mean()), p

    # ------------------------------------------------------------------------------------ io
    def state_dict(self):
        return dict(super().state_dict(), rng_offset=self.rng_offset())

    def load_state_dict(self, sd):
        with torch.cuda.stream(self.ctx.stream):
            self.rng_state.copy_(torch.tensor([int(sd["rng_offset"]), 0], dtype=torch.int64))
        super().load_state_dict(sd)

    def save_asset(self, path):
        """The eight arrays under the asset's keys, as MnistLabelClassifier(path) reads them."""
        with open(path, "wb") as f:
            np.savez(f, **{n: self.P.get(n) for n in self.P.names})


def asset_n_classes(asset):
    """Class count of a weight asset (the width of its last dense layer); reads the file only, needs no GPU."""
    import os
    if not os.path.exists(asset):
        raise RuntimeError("MNIST label-classifier weights missing: %s (python -m rcgan_amd.train_mnist_classifier writes them)" % asset)
    with np.load(asset) as z:
        missing = [n for n in NAMES if n not in z.files]
        if missing:
            raise RuntimeError("%s is not an MNIST label-classifier asset: no %s" % (asset, ", ".join(missing)))
        return int(z["fc2|w"].shape[1])


class MnistLabelClassifier:
    """The trained classifier behind ``train_mnist.py --label_classifier PATH``: ``predict`` is a predict_fn for
    eval_mnist.generated_label_accuracy (float [n,28,28,1] in [0, 1], any n -> n class indices)."""
    FEATURE_DIM = FEATURE_DIM

    def __init__(self, asset, device=0):
        K = asset_n_classes(asset)
        self.ctx = ctx = Context(device, "f32", arena_bytes=1 << 30, ws_bytes=1 << 28)
        want = dict(variable_shapes(K))
        self.w = {}
        with np.load(asset) as z:
            for k in NAMES:
                a = np.ascontiguousarray(z[k], np.float32)
                if a.shape != want[k]:
                    raise RuntimeError("%s: %s has shape %s, expected %s" % (asset, k, a.shape, want[k]))
                t = ctx.persistent(a.shape, L.F32)
                with torch.cuda.stream(ctx.stream):
                    ctx.view(t).copy_(torch.from_numpy(a))
                t.name = k.replace("|", "/")
                self.w[t.name] = t
        ctx.sync()

    @property
    def n_classes(self):
        return self.w["fc2/w"].shape[1]

    def softmax(self, images, batch=1000):
        """float [n,28,28,1] in [0, 1] -> softmax [n,K] float32 (no dropout)."""
        return _softmax(self.ctx, self.w, images, batch)

    def predict(self, images):
        """The arg-max class of each image, lowest index on ties."""
        return np.argmax(self.softmax(images), axis=1)

    __call__ = predict

    def features(self, images, batch=1000):
        """The [n,1024] feature tensor the last dense layer reads (after the ReLU, no dropout)."""
        out = []
        _forward_chunks(self.ctx, self.w, images, batch, lambda lg, ft, lo, n: out.append(self.ctx.download(ft).copy()))
        return np.concatenate(out, axis=0) if out else np.zeros((0, FEATURE_DIM), np.float32)

    def close(self):
        self.ctx.close()
