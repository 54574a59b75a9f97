"""Training the label classifier that generated-label accuracy is scored with (eval_cifar.LabelClassifier) on the engine's own
kernels, for any class count: the pre-activation ResNet-32 of ``eval_cifar.classifier_logits`` (the one forward pass both classes
run), sparse softmax cross-entropy, tf.train.MomentumOptimizer with L2 weight decay on the filters and the dense weight, and the
usual CIFAR input pipeline (random translation by up to ``pad`` pixels, random mirror) over a training set that lives on the
device.  fp32 activations, single GPU.

Batch norm uses the moments of the batch in hand in training AND in evaluation: ``generated_label_accuracy`` feeds its 1000
samples as one batch with no moving statistics, so the network is trained the way it will be used.  ``save_asset`` writes the
``.npz`` that ``LabelClassifier(asset=path)`` reads.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops as O
from .data import check_confusion_matrix
from .eval_cifar import BLOCKS, BN_EPS, STAGES, check_images, classifier_logits
from .runtime import Context, ParamGroup, check_f32_matmul_precision


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


class LabelClassifierTrainer:
    def __init__(self, n_classes, batch_size=128, momentum=0.9, weight_decay=1e-4, nesterov=False, pad=4, device=0, seed=0,
                 use_graphs=True, variables=None, f32_matmul_precision="highest", arena_bytes=6 << 30, confusion_matrix=None):
        """confusion_matrix: None trains on the labels as they are (sparse softmax cross-entropy).  A [K,K] row-stochastic matrix
        C[clean, noisy] declares the labels NOISY: the step then uses the forward-corrected loss -log((softmax(z) . C)[label]) (Patrini
        et al. 2017), under which the soft-max estimates the CLEAN posterior, and ``recover_labels`` becomes available."""
        self.f32_matmul_precision = check_f32_matmul_precision(f32_matmul_precision, "f32")
        specs = variables if variables is not None else create_classifier_variables(seed, n_classes)
        shapes = {n: tuple(s) for n, s, _ in specs}
        if shapes.get("fc|fc_weights") != (64, n_classes):
            raise ValueError("variables hold a %s dense layer, expected (64, %d)" % (shapes.get("fc|fc_weights"), n_classes))
        self.K, self.B = int(n_classes), int(batch_size)
        self.momentum, self.weight_decay, self.nesterov, self.pad = float(momentum), float(weight_decay), bool(nesterov), int(pad)
        self.use_graphs = bool(use_graphs)
        self.ctx = ctx = Context(device, "f32", arena_bytes=arena_bytes, ws_bytes=1 << 28)
        ctx.set_f32_matmul_precision(self.f32_matmul_precision)
        self.P = ParamGroup(ctx, specs)          # value / grad slabs; the Adam ``m`` slab holds the momentum accumulator
        names = self.P.names
        self.decay_count = self.P.offsets[names[N_DECAYED]]     # everything in front of the first gamma (slab padding is zero and stays zero)
        self.w = {}
        for n in names:
            p = self.P.param(n)
            p.req = True
            self.w[n.replace("|", "/")] = p
        B = self.B
        self.x = ctx.persistent((B, 32, 32, 3), L.F32, fill=0.0)
        self.labels = ctx.persistent((B,), "i32", fill=0)
        self.draws = ctx.persistent((4 * B,), "i32", fill=0)     # [index (B) | shift_flip (B x 3)]: one upload per step
        with torch.cuda.stream(ctx.stream):
            self.hyper = torch.zeros(2, dtype=torch.float32, device=ctx.device)      # {lr, step}: the update reads lr
        self.loss_acc, self.n_correct = self.P.scalar(0), self.P.scalar(1)
        # the transposed confusion matrix (ct[noisy, clean]: the layout the loss kernel reads) in a buffer a captured step keeps addressing
        self.ct = self.confusion_matrix = None
        if confusion_matrix is not None:
            self.ct = ctx.persistent((self.K, self.K), L.F32, fill=0.0)
            self.set_confusion_matrix(confusion_matrix)
        self.images = self.labels_all = None
        self.n_images = 0
        self.rs = np.random.RandomState(seed + 1)                # the draws of the input pipeline
        self._order, self._at = None, 0
        self.steps = 0
        self._graph, self._rehearsed = None, False
        ctx.sync()

    def set_confusion_matrix(self, C_matrix):
        """Overwrite the confusion matrix in place (validated on the host: entries >= 0, rows summing to 1 within 1e-6); a captured step
        reads the new one from its next launch on.  Only for a trainer that was built with one."""
        if self.ct is None:
            raise RuntimeError("this trainer was built without a confusion matrix (plain cross-entropy)")
        Cm = check_confusion_matrix(C_matrix, self.K)
        self.ctx.upload(np.ascontiguousarray(Cm.T), L.F32, out=self.ct)
        self.confusion_matrix = Cm

    # ------------------------------------------------------------------------------------ data
    def load_data(self, images_chw_u8, labels):
        """The training set onto the device: images [N,3072] bytes (CHW rows, as the CIFAR pickles hold them), labels [N]."""
        img = np.ascontiguousarray(np.asarray(images_chw_u8).reshape(len(labels), 3072).astype(np.uint8))
        lab = np.ascontiguousarray(np.asarray(labels).astype(np.int32))
        if lab.min() < 0 or lab.max() >= self.K:
            raise ValueError("labels outside [0, %d)" % self.K)
        if self._graph is not None:
            self.ctx.check(self.ctx.lib.rcgan_graph_destroy(self.ctx.h, self._graph))      # the captured step addresses the old buffers
            self._graph = None
        with torch.cuda.stream(self.ctx.stream):
            self.images = torch.from_numpy(img).to(self.ctx.device)
            self.labels_all = torch.from_numpy(lab).to(self.ctx.device)
        self.n_images = len(lab)
        self._order, self._at = None, 0
        self.ctx.sync()

    def _draw_index(self):
        """The next batch of a shuffled pass over the training set (a fresh permutation per pass, the tail carried over)."""
        out = []
        while len(out) < self.B:
            if self._order is None or self._at >= len(self._order):
                self._order, self._at = self.rs.permutation(self.n_images), 0
            take = self._order[self._at:self._at + self.B - len(out)]
            self._at += len(take)
            out.extend(take.tolist())
        return np.asarray(out, np.int32)

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
        logits = classifier_logits(ctx, self.w, self.x)
        if self.ct is None:
            O.softmax_xent(ctx, logits, self.labels, 1.0, self.loss_acc, self.n_correct)
        else:
            O.softmax_xent_forward(ctx, logits, self.labels, self.ct, 1.0, self.loss_acc, self.n_correct)
        ctx.backward()
        ctx.check(ctx.lib.rcgan_sgd_momentum(ctx.h, self.P.count, self.decay_count, self.P.value.data_ptr(), self.P.grad.data_ptr(),
                                             self.P.m.data_ptr(), self.hyper.data_ptr(), self.momentum, self.weight_decay,
                                             1 if self.nesterov else 0, 1.0))

    def step(self, lr, index=None, shift_flip=None):
        """One training step on a batch of the loaded set: sample ``index`` [B], each translated / mirrored by ``shift_flip`` [B,3] =
        (down, right, mirror); both drawn from the trainer's own numpy stream when not given."""
        ctx, B = self.ctx, self.B
        if self.images is None:
            raise RuntimeError("load_data() first")
        index = self._draw_index() if index is None else np.asarray(index, np.int32).reshape(-1)
        sf = self._draw_shift_flip() if shift_flip is None else np.asarray(shift_flip, np.int32).reshape(-1, 3)
        if index.shape != (B,) or sf.shape != (B, 3):
            raise ValueError("index %s / shift_flip %s for batch size %d" % (index.shape, sf.shape, B))
        if index.min() < 0 or index.max() >= self.n_images:
            raise ValueError("index outside [0, %d)" % self.n_images)
        if np.abs(sf[:, :2]).max() > self.pad:
            raise ValueError("shift beyond pad = %d" % self.pad)
        ctx.upload(np.concatenate([index, sf.reshape(-1)]), out=self.draws)
        ctx.check(ctx.lib.rcgan_set2_f32(ctx.h, self.hyper.data_ptr(), float(lr), float(self.steps)))
        if not self.use_graphs or not self._rehearsed:
            # eager: always without graphs, and the very first step with them (module loads; it also grows the fp32 path's hidden scratch)
            self._body()
            self._rehearsed = True
        else:
            if self._graph is None:
                # the fp32 convolutions keep split-reduction partials in a hidden scratch that cannot grow inside a capture.  The
                # eager rehearsal above ran these very shapes and has grown it already; the reservation is the documented upper bound
                # of that scratch for ANY shape (16 MiB, include/rcgan_hip.h: capture contract), independent of the batch size, so
                # the capture does not hinge on the rehearsal.  (The narrow data gradient's scratch is not used: no layer here
                # produces a gradient for <= 2 channels.)
                ctx.reserve_scratch(16 << 20)
                ctx.graph_begin()
                try:
                    self._body()
                except BaseException:
                    ctx.graph_abort()
                    raise
                self._graph = ctx.graph_end()
            ctx.graph_launch(self._graph)
        self.P.version += 1
        self.steps += 1

    def losses(self):
        """(mean loss, accuracy) of the last step's batch, both before its update."""
        return float(self.ctx.download(self.loss_acc)[0]), float(self.ctx.download(self.n_correct)[0]) / self.B

    def get_grads(self):
        return {n: self.P.get(n, "grad") for n in self.P.names}

    # ------------------------------------------------------------------------------------ evaluation
    def evaluate(self, images, labels, batch=1000):
        """Accuracy and softmax on [n,32,32,3] images of raw pixel values 0..255, ``batch`` at a time, each batch normalised with its
        own moments: the protocol of generated_label_accuracy (and the launches of LabelClassifier.softmax)."""
        ctx = self.ctx
        x = check_images(images)
        out = []
        rec, ctx.recording = ctx.recording, False
        try:
            for lo in range(0, len(x), batch):
                ctx.new_step()
                logits = classifier_logits(ctx, self.w, ctx.upload(x[lo:lo + batch], L.F32))
                out.append(ctx.download(O.softmax_rows(ctx, logits)))
        finally:
            ctx.recording = rec
        p = np.concatenate(out, axis=0)
        return float((np.argmax(p, axis=1) == np.asarray(labels)).mean()), p

    def recover_labels(self, images, noisy_labels, batch=1000):
        """Label recovery: the posterior over the CLEAN label of each image given its noisy one, post[y] ~ softmax(z)[y] C[y, noisy], and
        its arg-max (lowest index on ties) -> (recovered [n] int32, posterior [n,K] fp32).  Images as ``evaluate`` takes them, under the
        same protocol: ``batch`` at a time, each batch on its own batch-norm moments, recording off.  A label outside [0, K), or one no
        class can emit under C, gives recovered = -1 and a zero posterior row."""
        if self.ct is None:
            raise RuntimeError("recover_labels needs the confusion matrix the trainer was built with")
        ctx = self.ctx
        x = check_images(images)
        noisy = np.ascontiguousarray(np.asarray(noisy_labels).reshape(-1).astype(np.int32))
        if len(noisy) != len(x):
            raise ValueError("%d labels for %d images" % (len(noisy), len(x)))
        rec_out, post_out = [], []
        rec, ctx.recording = ctx.recording, False
        try:
            for lo in range(0, len(x), batch):
                ctx.new_step()
                n = len(x[lo:lo + batch])
                logits = classifier_logits(ctx, self.w, ctx.upload(x[lo:lo + batch], L.F32))
                post, got = ctx.empty((n, self.K), L.F32), ctx.empty((n,), "i32")
                O.softmax_xent_forward(ctx, logits, ctx.upload(noisy[lo:lo + batch]), self.ct, 1.0, None, None, post, got)
                rec_out.append(ctx.download(got).copy())
                post_out.append(ctx.download(post).copy())
        finally:
            ctx.recording = rec
        return np.concatenate(rec_out, axis=0), np.concatenate(post_out, axis=0)

    # ------------------------------------------------------------------------------------ io
    def state_dict(self):
        return dict(value={n: self.P.get(n) for n in self.P.names}, momentum={n: self.P.get(n, "m") for n in self.P.names},
                    steps=self.steps, rng=self.rs.get_state(), order=None if self._order is None else self._order.copy(), at=self._at)

    def load_state_dict(self, sd):
        for n in self.P.names:
            self.P.set(n, sd["value"][n])
            self.P.set(n, sd["momentum"][n], "m")
        self.steps = int(sd["steps"])
        self.rs.set_state(sd["rng"])
        self._order, self._at = (None if sd["order"] is None else np.asarray(sd["order"]).copy()), int(sd["at"])
        self.ctx.sync()

    def save_asset(self, path):
        """The weights as LabelClassifier(asset=path) reads them (the 95 float arrays under the asset's keys, plus the batch-norm
        epsilon scalars the reference's graph carries)."""
        arrs = {n: self.P.get(n) for n in self.P.names}
        for n in self.P.names:
            if n.endswith("|gamma"):
                arrs[n[:-len("gamma")] + "batchnorm|add|y"] = np.float32(BN_EPS)
        with open(path, "wb") as f:
            np.savez(f, **arrs)

    def close(self):
        self.ctx.close()
