"""Generated-label accuracy (gan_resnet.py:424-455, 847-861, 995-1005): how often a frozen CIFAR-10 classifier agrees
with the label the generator was conditioned on.

The reference imports ``resnet-110/graph_optimized.pb`` into a TensorFlow session.  Here the same network -- decoded from
that file without TensorFlow by scripts/extract_label_classifier.py into assets/cifar_label_classifier.npz -- runs on the
engine's own kernels in fp32: a pre-activation ResNet-32 (conv0 3->16, three stages of five basic blocks at 16/32/64
channels, stride-2 first conv in stages 2 and 3 with the option-A shortcut = 2x2 average pool + zero channel padding),
every batch norm on the moments of the evaluated batch itself (eps 1e-3, no moving statistics), ReLU, global average
pool, 64->K dense layer, softmax (K = 10 for the committed asset; classifier.py trains the same network for any K).  Inputs are the raw integer pixels 0..255 in NHWC, all 1000 samples in ONE batch
(the batch statistics depend on it), exactly as ``generated_label_accuracy`` feeds them.

The Frechet distance (frechet.py) reads the same network's pooled 64-wide feature under FROZEN statistics instead:
``LabelClassifier.calibrate`` takes the 31 (mean, variance) pairs once from a batch of real images, ``features`` applies them to
every image through inference-mode batch norm, so that a sample's feature does not depend on what else is in its batch.
"""
import os

import numpy as np

from . import _lib as L
from . import ops as O
from .runtime import Context

ASSET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "cifar_label_classifier.npz")
BN_EPS = 1e-3
STAGES, BLOCKS = 3, 5


def bn_layer_names():
    """The 31 batch norms of the network in execution order ('/'-separated, as the weight dictionaries are keyed)."""
    out = ["conv0"]
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            if not (s == 1 and b == 0):
                out.append(p + "/conv1_in_block")
            out.append(p + "/conv2_in_block")
    return out + ["fc"]


def classifier_logits(ctx, w, x, frozen=None, stats_out=None, features=False):
    """The forward pass of the label classifier, written once: x [n,32,32,3] fp32 device tensor of raw pixel values, w = {name: device
    tensor} under the asset's names ('/'-separated) -> logits [n,K].  Every batch norm uses the moments of this batch.  Recorded on the
    tape when ctx.recording is on and the weights require gradients (classifier.LabelClassifierTrainer), forward only otherwise.
    features: return the pooled [n,64] feature the dense layer reads instead of the logits.
    stats_out = {layer: (mean, rstd)} device tensors: the batch-moment pass leaves every layer's moments there (calibration).
    frozen = {layer: (mean, biased variance)}: inference-mode batch norm with those pairs -- a sample's output then does not
    depend on what else is in its batch (the feature pass of the Frechet distance)."""
    conv = lambda t, name, stride=1: O.conv2d(ctx, t, O.Weight(ctx, w[name + "/conv"]), None, 3, stride=stride)
    if frozen is not None:
        bn_relu = lambda t, name: O.batch_norm_infer(ctx, t, w[name + "/gamma"], w[name + "/beta"], frozen[name][0], frozen[name][1],
                                                     act=L.ACT_RELU, eps=BN_EPS)
    elif stats_out is not None:
        bn_relu = lambda t, name: O.batch_norm_act(ctx, t, w[name + "/gamma"], w[name + "/beta"], act=L.ACT_RELU, eps=BN_EPS,
                                                   stats_out=stats_out[name])
    else:
        bn_relu = lambda t, name: O.batch_norm_act(ctx, t, w[name + "/gamma"], w[name + "/beta"], act=L.ACT_RELU, eps=BN_EPS)
    h = bn_relu(conv(x, "conv0"), "conv0")
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            down = b == 0 and s > 1
            t = h if (s == 1 and b == 0) else bn_relu(h, p + "/conv1_in_block")
            c1 = conv(t, p + "/conv1_in_block", stride=2 if down else 1)
            c2 = conv(bn_relu(c1, p + "/conv2_in_block"), p + "/conv2_in_block")
            # option-A shortcut of the down-sampling blocks: AvgPool 2x2 + Pad channels (C/2 each side), one launch
            h = O.add(ctx, c2, O.shortcut_a(ctx, h) if down else h)
    feat = O.act_meanhw(ctx, bn_relu(h, "fc"), L.ACT_NONE)
    if features:
        return feat
    return O.linear(ctx, feat, O.Weight(ctx, w["fc/fc_weights"]), w["fc/fc_bias"])


def check_images(images):
    x = np.ascontiguousarray(np.asarray(images, np.float32))
    if x.ndim != 4 or x.shape[1:] != (32, 32, 3):
        raise ValueError("expected [n,32,32,3] images, got %s" % (x.shape,))
    return x


def asset_n_classes(asset):
    """Class count of a weight asset (the width of its dense layer); reads the file only, needs no GPU."""
    if not os.path.exists(asset):
        raise RuntimeError("label-classifier weights missing: %s" % asset)
    with np.load(asset) as z:
        return int(z["fc|fc_weights"].shape[1])


class LabelClassifier:
    def __init__(self, device=0, arena_bytes=5 << 30, asset=ASSET):
        if not os.path.exists(asset):
            raise RuntimeError("label-classifier weights missing: %s (scripts/extract_label_classifier.py writes them)" % asset)
        self.ctx = ctx = Context(device, "f32", arena_bytes=arena_bytes, ws_bytes=1 << 28)
        z = np.load(asset)
        self.w = {}
        for k in z.files:
            a = z[k]
            if a.dtype.kind != "f" or a.ndim == 0:
                continue                                   # reduction indices, paddings, eps scalars
            t = ctx.persistent(a.shape, L.F32)
            ctx.view(t).copy_(__import__("torch").from_numpy(np.ascontiguousarray(a, np.float32)))
            t.name = k.replace("|", "/")
            self.w[t.name] = t
        ctx.sync()

    @property
    def n_classes(self):
        return self.w["fc/fc_weights"].shape[1]

    def softmax(self, images):
        """images: [n,32,32,3] raw pixel values 0..255 (any numeric dtype).  -> softmax [n,K] float32."""
        ctx = self.ctx
        x = check_images(images)
        ctx.new_step()
        rec, ctx.recording = ctx.recording, False
        try:
            logits = classifier_logits(ctx, self.w, ctx.upload(x, L.F32))
            return ctx.download(O.softmax_rows(ctx, logits))
        finally:
            ctx.recording = rec

    # ---------------------------------------------------------------- frozen-statistics features (frechet.py)
    FEATURE_DIM = 64

    def _forward_only(self, fn):
        ctx = self.ctx
        ctx.new_step()
        rec, ctx.recording = ctx.recording, False
        try:
            return fn()
        finally:
            ctx.recording = rec

    def batch_moment_features(self, images):
        """The pooled [n,64] feature with every batch norm on the moments of THIS batch (what ``softmax`` feeds its dense layer):
        depends on what else is in the batch -- the metric uses ``features``; this is the other path, for comparison."""
        ctx = self.ctx
        x = check_images(images)
        return self._forward_only(lambda: ctx.download(classifier_logits(ctx, self.w, ctx.upload(x, L.F32), features=True)))

    def calibrate(self, images):
        """One batch-moment pass over ``images`` (the calibration batch, [n,32,32,3] raw pixels) that keeps the 31 (mean, biased
        variance) pairs on the device for ``features``.  The pairs come from rcgan_bn_stats -- the very launch that normalises the
        calibration batch -- as its mean and 1 / rstd^2 - eps (formed in float64 on the host, clipped at 0, stored as fp32); the
        ``moving=`` path is not used (its variance is the unbiased one and would need the n / (n - 1) factor taken out again).
        -> the batch-moment features [n,64] of the calibration batch."""
        ctx = self.ctx
        x = check_images(images)
        names = bn_layer_names()
        if getattr(self, "_stats", None) is None:
            self._stats = {k: (ctx.persistent(self.w[k + "/gamma"].shape, L.F32), ctx.persistent(self.w[k + "/gamma"].shape, L.F32))
                           for k in names}
            self._frozen = {k: (ctx.persistent(self.w[k + "/gamma"].shape, L.F32), ctx.persistent(self.w[k + "/gamma"].shape, L.F32))
                            for k in names}
        feat = self._forward_only(lambda: ctx.download(classifier_logits(ctx, self.w, ctx.upload(x, L.F32), stats_out=self._stats,
                                                                         features=True)))
        pairs = {}
        for k in names:
            mean, rstd = ctx.download(self._stats[k][0]), ctx.download(self._stats[k][1]).astype(np.float64)
            pairs[k] = (mean.astype(np.float32), np.maximum(1.0 / (rstd * rstd) - float(np.float32(BN_EPS)), 0.0).astype(np.float32))
        self.set_calibration(pairs)
        return feat

    def set_calibration(self, pairs):
        """Install calibration pairs {layer: (mean, biased variance)} (numpy, as ``calibration()`` returns them)."""
        ctx = self.ctx
        names = bn_layer_names()
        if getattr(self, "_frozen", None) is None:
            self._stats = None
            self._frozen = {k: (ctx.persistent(self.w[k + "/gamma"].shape, L.F32), ctx.persistent(self.w[k + "/gamma"].shape, L.F32))
                            for k in names}
        for k in names:
            for dst, a in zip(self._frozen[k], pairs[k]):
                a = np.ascontiguousarray(a, np.float32)
                if a.shape != dst.shape:
                    raise ValueError("calibration pair of %s has shape %s, expected %s" % (k, a.shape, dst.shape))
                ctx.upload(a, L.F32, out=dst)
        ctx.sync()
        self._pairs = {k: (np.array(pairs[k][0], np.float32), np.array(pairs[k][1], np.float32)) for k in names}

    def calibration(self):
        """{layer: (mean, biased variance)} float32 numpy, or None before ``calibrate`` / ``set_calibration``."""
        return getattr(self, "_pairs", None)

    def features(self, images, labels=None, moments=None, chunk=1000):
        """The pooled [n,64] fp32 feature of every image under the FROZEN statistics of ``calibrate``, in chunks of ``chunk`` images
        (a tail chunk of any size is legal: a frozen feature does not depend on what else is in its batch; across batch SIZES the
        convolutions may take another route, which moves fp32 rounding only).  moments (frechet.ClassMoments): every
        chunk's features go to its kernel on the device with ``labels`` (None: one class) and nothing is downloaded -> None;
        otherwise -> the features as float32 numpy."""
        if getattr(self, "_pairs", None) is None:
            raise RuntimeError("LabelClassifier.features needs calibrate() (or set_calibration()) first")
        if chunk < 1:
            raise ValueError("chunk %d: at least one image" % chunk)
        ctx = self.ctx
        x = check_images(images)
        if labels is not None:
            labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
            if len(labels) != len(x):
                raise ValueError("%d labels for %d images" % (len(labels), len(x)))
        out = None if moments is not None else np.empty((len(x), self.FEATURE_DIM), np.float32)

        def one(lo):
            xs = x[lo:lo + chunk]
            feat = classifier_logits(ctx, self.w, ctx.upload(xs, L.F32), frozen=self._frozen, features=True)
            if moments is None:
                out[lo:lo + len(xs)] = ctx.download(feat)
            else:
                moments.add(feat, None if labels is None else ctx.upload(labels[lo:lo + len(xs)]))
        for lo in range(0, len(x), chunk):
            self._forward_only(lambda: one(lo))
        return out

    def close(self):
        self.ctx.close()


class TemplateClassifier:
    """Stand-in label classifier for the "templates" synthetic images (data.synthetic_cifar(kind="templates")): the class of an
    image is the nearest of the ten class patterns in the pre-squash domain, atanh(pixel) vs 0.6 * template -- the maximum-
    likelihood rule of that generative model up to the noise covariance; 99.9 % correct on the synthetic real images
    (tests/test_host_cpu.py).  Host numpy: evaluation of a synthetic stand-in, not part of the training step.  Same interface as
    ``LabelClassifier`` (``softmax`` returns a one-hot row per image) so ``generated_label_accuracy`` takes either."""

    def __init__(self, device=0):
        from . import data as D
        self.t = (0.6 * D.class_templates()).transpose(0, 2, 3, 1).reshape(10, -1).astype(np.float32)     # HWC rows

    def softmax(self, images):
        x = np.asarray(images, np.float32)
        if x.ndim != 4 or x.shape[1:] != (32, 32, 3):
            raise ValueError("expected [n,32,32,3] images, got %s" % (x.shape,))
        a = np.arctanh(np.clip((x + 0.5) / 128.0 - 1.0, -0.999, 0.999)).reshape(len(x), -1)
        d = (a * a).sum(1, keepdims=True) - 2.0 * a.dot(self.t.T) + (self.t * self.t).sum(1)[None]
        out = np.zeros((len(x), 10), np.float32)
        out[np.arange(len(x)), d.argmin(1)] = 1.0
        return out

    def close(self):
        pass


def generated_label_accuracy(samples, labels, confusion_matrix=None, classifier=None, device=0):
    """gan_resnet.py:424-455.  samples int [n,32,32,3] in 0..255; labels int [n]; confusion_matrix (rcgan-u): labels are
    first mapped through the arg-max permutation of the learned matrix."""
    labels = np.asarray(labels)
    if confusion_matrix is not None:
        cm = np.asarray(confusion_matrix)
        perm = np.zeros_like(cm, dtype=int)
        perm[np.arange(cm.shape[0]), np.argmax(cm, axis=-1)] = 1
        onehot = np.zeros([labels.shape[0], cm.shape[0]], dtype=float)
        onehot[np.arange(labels.shape[0]), labels] = 1
        labels = np.argmax(onehot.dot(perm), axis=-1)
    own = classifier is None
    clf = LabelClassifier(device) if own else classifier
    try:
        softmax = clf.softmax(samples)
    finally:
        if own:
            clf.close()
    return float((labels == np.argmax(softmax, axis=-1)).astype(float).mean())
