"""Training the label classifier that generated-label accuracy is scored with (eval_cifar.LabelClassifier) on the engine's own
kernels, for any class count: the pre-activation ResNet-32 of ``eval_cifar.classifier_logits`` (the one forward pass both classes
run), sparse softmax cross-entropy, tf.train.MomentumOptimizer with L2 weight decay on the filters and the dense weight, and the
usual CIFAR input pipeline (random translation by up to ``pad`` pixels, random mirror) over a training set that lives on the
device.  fp32 activations, single GPU.

Batch norm uses the moments of the batch in hand in training AND in evaluation: ``generated_label_accuracy`` feeds its 1000
samples as one batch with no moving statistics, so the network is trained the way it will be used.  ``save_asset`` writes the
``.npz`` that ``LabelClassifier(asset=path)`` reads.

What this trainer shares with the MNIST one (the confusion matrix and the loss choice, the passes over the training set, the eager /
captured step, label recovery, the checkpoint) is ``label_trainer.LabelTrainer``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops as O
from .eval_cifar import BLOCKS, BN_EPS, STAGES, check_images, classifier_logits
from .label_trainer import LabelTrainer
from .runtime import check_f32_matmul_precision


def _layer_names():
    convs, bns = ["conv0"], ["conv0"]
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            convs += [p + "|conv1_in_block", p + "|conv2_in_block"]
            if not (s == 1 and b == 0):
                bns.append(p + "|conv1_in_block")
            bns.append(p + "|conv2_in_block")
    return convs, bns + ["fc"]


def create_classifier_variables(seed, n_classes):
    """[(name, shape, init)] of the 95 float arrays of the classifier's weight asset (its '|'-separated keys), the dense layer
    n_classes wide: He-normal filters (fan-out), gamma 1, beta 0, dense weight uniform +-1/8, bias 0.  The decayed variables
    (31 filters, the dense weight) come first, the gammas / betas / the dense bias after them."""
    if not 2 <= int(n_classes) <= L.MAX_CLASSES:
        raise ValueError("n_classes %r: 2..%d" % (n_classes, L.MAX_CLASSES))
    rs = np.random.RandomState(seed)
    convs, bns = _layer_names()
    specs, cin = [], 3
    for name in convs:
        cout = 16 if name == "conv0" else 16 << (int(name[4]) - 1)
        shape = (3, 3, cin, cout)
        specs.append((name + "|conv", shape, (rs.randn(*shape) * np.sqrt(2.0 / (9 * cout))).astype(np.float32)))
        cin = cout
    specs.append(("fc|fc_weights", (64, n_classes), rs.uniform(-0.125, 0.125, size=(64, n_classes)).astype(np.float32)))
    filt = {n: sh for n, sh, _ in specs}
    for name in bns:
        # conv0's batch norm follows its filter; inside a block each one normalises the INPUT of the filter it is named after (pre-activation)
        c = 64 if name == "fc" else filt[name + "|conv"][3 if name == "conv0" else 2]
        specs.append((name + "|gamma", (c,), np.ones(c, np.float32)))
        specs.append((name + "|beta", (c,), np.zeros(c, np.float32)))
    specs.append(("fc|fc_bias", (n_classes,), np.zeros(n_classes, np.float32)))
    return specs


N_DECAYED = 32      # the first variables of create_classifier_variables: 31 filters + the dense weight


class LabelClassifierTrainer(LabelTrainer):
    SLABS = (("momentum", "m"),)        # the Adam ``m`` slab holds the momentum accumulator
    _check_images = staticmethod(check_images)

    def __init__(self, n_classes, batch_size=128, momentum=0.9, weight_decay=1e-4, nesterov=False, pad=4, device=0, seed=0,
                 use_graphs=True, variables=None, f32_matmul_precision="highest", arena_bytes=6 << 30, confusion_matrix=None):
        """confusion_matrix: None trains on the labels as they are (sparse softmax cross-entropy).  A [K,K] row-stochastic matrix
        C[clean, noisy] declares the labels NOISY: the step then uses the forward-corrected loss -log((softmax(z) . C)[label]) (Patrini
        et al. 2017), under which the soft-max estimates the CLEAN posterior, and ``recover_labels`` becomes available."""
        check_f32_matmul_precision(f32_matmul_precision, "f32")
        specs = variables if variables is not None else create_classifier_variables(seed, n_classes)
        shapes = {n: tuple(s) for n, s, _ in specs}
        if shapes.get("fc|fc_weights") != (64, n_classes):
            raise ValueError("variables hold a %s dense layer, expected (64, %d)" % (shapes.get("fc|fc_weights"), n_classes))
        self.momentum, self.weight_decay, self.nesterov, self.pad = float(momentum), float(weight_decay), bool(nesterov), int(pad)
        super().__init__(specs, n_classes, batch_size, seed, use_graphs, f32_matmul_precision, confusion_matrix, device, arena_bytes)

    def _make_buffers(self):
        ctx, B = self.ctx, self.B
        self.decay_count = self.P.offsets[self.P.names[N_DECAYED]]     # everything in front of the first gamma (slab padding is zero and stays zero)
        self.x = ctx.persistent((B, 32, 32, 3), L.F32, fill=0.0)
        self.labels = ctx.persistent((B,), "i32", fill=0)
        self.draws = ctx.persistent((4 * B,), "i32", fill=0)     # [index (B) | shift_flip (B x 3)]: one upload per step
        with torch.cuda.stream(ctx.stream):
            self.hyper = torch.zeros(2, dtype=torch.float32, device=ctx.device)      # {lr, step}: the update reads lr

    # ------------------------------------------------------------------------------------ data
    def load_data(self, images_chw_u8, labels):
        """The training set onto the device: images [N,3072] bytes (CHW rows, as the CIFAR pickles hold them), labels [N]."""
        img = np.ascontiguousarray(np.asarray(images_chw_u8).reshape(len(labels), 3072).astype(np.uint8))
        self._install_data(img, np.ascontiguousarray(np.asarray(labels).astype(np.int32)), labels_on_device=True)

    def _draw_shift_flip(self):
        sf = np.zeros((self.B, 3), np.int32)
        if self.pad:
            sf[:, :2] = self.rs.randint(-self.pad, self.pad + 1, size=(self.B, 2))
        sf[:, 2] = self.rs.randint(2, size=self.B)
        return sf

    # ------------------------------------------------------------------------------------ step
    def _body(self):
        ctx, B = self.ctx, self.B
        ctx.new_step()
        self.P.zero_grad()
        ctx.check(ctx.lib.rcgan_augment_cifar(ctx.h, B, self.n_images, C.c_void_p(self.images.data_ptr()), C.c_void_p(self.labels_all.data_ptr()),
                                              C.c_void_p(self.draws.ptr), C.c_void_p(self.draws.ptr + 4 * B), self.pad, L.F32,
                                              C.c_void_p(self.x.ptr), C.c_void_p(self.labels.ptr)))
        self._loss(classifier_logits(ctx, self.w, self.x))
        ctx.backward()
        ctx.check(ctx.lib.rcgan_sgd_momentum(ctx.h, self.P.count, self.decay_count, self.P.value.data_ptr(), self.P.grad.data_ptr(),
                                             self.P.m.data_ptr(), self.hyper.data_ptr(), self.momentum, self.weight_decay,
                                             1 if self.nesterov else 0, 1.0))

    def step(self, lr, index=None, shift_flip=None):
        """One training step on a batch of the loaded set: sample ``index`` [B], each translated / mirrored by ``shift_flip`` [B,3] =
        (down, right, mirror); both drawn from the trainer's own numpy stream when not given."""
        ctx, B = self.ctx, self.B
        index = self._step_index(index)
        sf = self._draw_shift_flip() if shift_flip is None else np.asarray(shift_flip, np.int32).reshape(-1, 3)
        if index.shape != (B,) or sf.shape != (B, 3):
            raise ValueError("index %s / shift_flip %s for batch size %d" % (index.shape, sf.shape, B))
        self._check_index_range(index)
        if np.abs(sf[:, :2]).max() > self.pad:
            raise ValueError("shift beyond pad = %d" % self.pad)
        ctx.upload(np.concatenate([index, sf.reshape(-1)]), out=self.draws)
        ctx.check(ctx.lib.rcgan_set2_f32(ctx.h, self.hyper.data_ptr(), float(lr), float(self.steps)))
        self._run_step()

    # ------------------------------------------------------------------------------------ evaluation
    def _forward_chunks(self, images, batch, fn):
        """fn(logits, lo, n) over the images ``batch`` at a time, each batch normalised with its own moments, recording off."""
        ctx = self.ctx
        x = check_images(images)
        rec, ctx.recording = ctx.recording, False
        try:
            for lo in range(0, len(x), batch):
                ctx.new_step()
                part = x[lo:lo + batch]
                fn(classifier_logits(ctx, self.w, ctx.upload(part, L.F32)), lo, len(part))
        finally:
            ctx.recording = rec

    def evaluate(self, images, labels, batch=1000):
        """Accuracy and softmax on [n,32,32,3] images of raw pixel values 0..255, ``batch`` at a time, each batch normalised with its
        own moments: the protocol of generated_label_accuracy (and the launches of LabelClassifier.softmax)."""
        ctx, out = self.ctx, []
        self._forward_chunks(images, batch, lambda logits, lo, n: out.append(ctx.download(O.softmax_rows(ctx, logits))))
        p = np.concatenate(out, axis=0)
        return float((np.argmax(p, axis=1) == np.asarray(labels)).mean()), p

    # ------------------------------------------------------------------------------------ io
    def save_asset(self, path):
        """The weights as LabelClassifier(asset=path) reads them (the 95 float arrays under the asset's keys, plus the batch-norm
        epsilon scalars the reference's graph carries)."""
        arrs = {n: self.P.get(n) for n in self.P.names}
        for n in self.P.names:
            if n.endswith("|gamma"):
                arrs[n[:-len("gamma")] + "batchnorm|add|y"] = np.float32(BN_EPS)
        with open(path, "wb") as f:
            np.savez(f, **arrs)
