"""What the two on-engine label-classifier trainers share (classifier.LabelClassifierTrainer, mnist_classifier.MnistClassifierTrainer):
one fp32 context and parameter group, the confusion matrix of the forward-corrected loss and the choice between the two losses, the
shuffled passes over a training set that lives on the device, the step's eager / captured execution, label recovery and the
checkpoint.  A trainer adds its variables and their checks, its persistent buffers, ``load_data``, ``step`` (upload, hyper-parameters,
then ``_run_step``), ``_body``, ``_forward_chunks``, ``evaluate`` and ``save_asset``.
"""
import numpy as np
import torch

from . import _lib as L
from . import ops as O
from .data import check_confusion_matrix
from .runtime import Context, ParamGroup


class LabelTrainer:
    SLABS = ()      # ((checkpoint key, ParamGroup slab), ...): the optimiser state a checkpoint carries beside "value"

    def __init__(self, specs, n_classes, batch_size, seed, use_graphs, f32_matmul_precision, confusion_matrix, device, arena_bytes):
        self.K, self.B = int(n_classes), int(batch_size)
        self.f32_matmul_precision, self.use_graphs = f32_matmul_precision, bool(use_graphs)
        self.ctx = ctx = Context(device, "f32", arena_bytes=arena_bytes, ws_bytes=1 << 28)
        ctx.set_f32_matmul_precision(f32_matmul_precision)
        self.P = ParamGroup(ctx, specs)
        self.w = {}
        for n in self.P.names:
            p = self.P.param(n)
            p.req = True
            self.w[n.replace("|", "/")] = p
        self._make_buffers()
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
    def _install_data(self, img, lab, labels_on_device):
        """The tail of load_data: img [N, row] as the step's gather reads it, lab [N] int32."""
        if lab.min() < 0 or lab.max() >= self.K:
            raise ValueError("labels outside [0, %d)" % self.K)
        if self._graph is not None:
            self.ctx.check(self.ctx.lib.rcgan_graph_destroy(self.ctx.h, self._graph))      # the captured step addresses the old buffers
            self._graph = None
        with torch.cuda.stream(self.ctx.stream):
            self.images = torch.from_numpy(img).to(self.ctx.device)
            self.labels_all = torch.from_numpy(lab).to(self.ctx.device) if labels_on_device else lab
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

    def _step_index(self, index):
        """The sample indices of a step: the caller's, flattened, or the next batch of the trainer's own numpy stream."""
        if self.images is None:
            raise RuntimeError("load_data() first")
        return self._draw_index() if index is None else np.asarray(index, np.int32).reshape(-1)

    def _check_index_range(self, index):
        if index.min() < 0 or index.max() >= self.n_images:
            raise ValueError("index outside [0, %d)" % self.n_images)

    # ------------------------------------------------------------------------------------ step
    def _loss(self, logits):
        if self.ct is None:
            O.softmax_xent(self.ctx, logits, self.labels, 1.0, self.loss_acc, self.n_correct)
        else:
            O.softmax_xent_forward(self.ctx, logits, self.labels, self.ct, 1.0, self.loss_acc, self.n_correct)

    def _run_step(self):
        """_body() once: eagerly without graphs and on the very first step with them (module loads; it also grows the fp32 path's hidden
        scratch), captured on the second, replayed from then on."""
        ctx = self.ctx
        if not self.use_graphs or not self._rehearsed:
            self._body()
            self._rehearsed = True
        else:
            if self._graph is None:
                # the fp32 convolutions keep split-reduction partials in a hidden scratch that cannot grow inside a capture.  The
                # eager rehearsal above ran these very shapes and has grown it already; the reservation is the documented upper bound
                # of that scratch for ANY shape (16 MiB, include/rcgan_hip.h: capture contract), independent of the batch size, so
                # the capture does not hinge on the rehearsal.  (The narrow data gradient's scratch is not used: no layer of either
                # network produces a gradient for <= 2 channels -- the first convolution's input is the data.)
                self._graph = ctx.capture(self._body, reserve=16 << 20)
            ctx.graph_launch(self._graph)
        self.P.version += 1
        self.steps += 1

    def losses(self):
        """(mean loss, accuracy) of the last step's batch, both before its update (and under its dropout mask, where there is one)."""
        return float(self.ctx.download(self.loss_acc)[0]), float(self.ctx.download(self.n_correct)[0]) / self.B

    def get_grads(self):
        return {n: self.P.get(n, "grad") for n in self.P.names}

    # ------------------------------------------------------------------------------------ evaluation
    def recover_labels(self, images, noisy_labels, batch=1000):
        """Label recovery: the posterior over the CLEAN label of each image given its noisy one, post[y] ~ softmax(z)[y] C[y, noisy], and
        its arg-max (lowest index on ties) -> (recovered [n] int32, posterior [n,K] fp32).  Images as ``evaluate`` takes them, under the
        same protocol (_forward_chunks: ``batch`` at a time, recording off).  A label outside [0, K), or one no class can emit under C,
        gives recovered = -1 and a zero posterior row."""
        if self.ct is None:
            raise RuntimeError("recover_labels needs the confusion matrix the trainer was built with")
        ctx = self.ctx
        x = self._check_images(images)
        noisy = np.ascontiguousarray(np.asarray(noisy_labels).reshape(-1).astype(np.int32))
        if len(noisy) != len(x):
            raise ValueError("%d labels for %d images" % (len(noisy), len(x)))
        rec_out, post_out = [], []

        def one(logits, lo, n):
            post, got = ctx.empty((n, self.K), L.F32), ctx.empty((n,), "i32")
            O.softmax_xent_forward(ctx, logits, ctx.upload(noisy[lo:lo + n]), self.ct, 1.0, None, None, post, got)
            rec_out.append(ctx.download(got).copy())
            post_out.append(ctx.download(post).copy())
        self._forward_chunks(x, batch, one)
        return np.concatenate(rec_out, axis=0), np.concatenate(post_out, axis=0)

    # ------------------------------------------------------------------------------------ io
    def state_dict(self):
        slab = lambda which: {n: self.P.get(n, which) for n in self.P.names}
        return dict(value=slab("value"), **{key: slab(which) for key, which in self.SLABS}, steps=self.steps, rng=self.rs.get_state(),
                    order=None if self._order is None else self._order.copy(), at=self._at)

    def load_state_dict(self, sd):
        for n in self.P.names:
            self.P.set(n, sd["value"][n])
            for key, which in self.SLABS:
                self.P.set(n, sd[key][n], which)
        self.steps = int(sd["steps"])
        self.rs.set_state(sd["rng"])
        self._order, self._at = (None if sd["order"] is None else np.asarray(sd["order"]).copy()), int(sd["at"])
        self.ctx.sync()

    def close(self):
        self.ctx.close()
