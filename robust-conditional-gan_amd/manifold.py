"""Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between two image sets,
pooled and per class, on the 64-wide pooled feature of the label classifier -- the feature the Frechet distance (frechet.py) reads,
under the same calibration.  Where one Frechet number per class mixes the two failures of a conditional GAN trained on noisy labels,
these four split them: precision and density fall when samples generated for class y leave the real manifold of class y (class
mixing, low fidelity); recall and coverage fall when parts of the real class y have no generated sample near them (mode dropping).

With g the generated rows and r the real rows of one segment (the whole set, or one class), k-NN radii taken WITHIN each set:
  precision = mean_g [ g lies in the ball of at least one r ]        recall   = mean_r [ r lies in the ball of at least one g ]
  density   = sum_g #{ real balls that contain g } / (k n_g)         coverage = mean_r [ the nearest g is inside r's own ball ]

The pairwise part never exists as a matrix: csrc/knn.hip computes the radii (``knn_radius``) and, per query row, the number of balls
that contain it and the distance to its nearest neighbour (``ball_query``); only those vectors are downloaded and everything after
them (``metrics``) is float64 numpy on the host.

The numbers are built around the engine's own small classifier: they are NOT comparable with published Inception / VGG values.

Stand-alone:  python -m rcgan_amd.manifold --real a.npz --generated b.npz [--k 5]   (each file: ``images`` [n,32,32,3] or [n,3072]
CHW rows of raw pixels 0..255, ``labels`` [n]) prints the same numbers as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import (N_CALIBRATION, FeatureEvaluator, FeatureSet, as_nhwc, check_rows, download, permuted_labels,  # noqa: F401
                         standalone)                    # (FeatureSet, as_nhwc, permuted_labels: re-exported for the callers of this module)

METRICS = ("precision", "recall", "density", "coverage")
MAX_K, MAX_SEGMENTS = 16, 1024          # the kernel's bounds on k and on the number of segments (include/rcgan_hip.h)


def metrics(count_g, count_r, nearest2_r, radius2_r, k):
    """The four numbers of one segment, float64.  count_g [n_g]: real balls around each generated row; count_r [n_r]: generated balls
    around each real row; nearest2_r [n_r]: squared distance from each real row to its nearest generated row; radius2_r [n_r]: each
    real row's own squared k-NN radius among the real rows.  An empty side gives nan."""
    count_g, count_r = np.asarray(count_g, np.float64).reshape(-1), np.asarray(count_r, np.float64).reshape(-1)
    nearest2_r, radius2_r = np.asarray(nearest2_r, np.float64).reshape(-1), np.asarray(radius2_r, np.float64).reshape(-1)
    if nearest2_r.shape != count_r.shape or radius2_r.shape != count_r.shape:
        raise ValueError("metrics: %s counts, %s nearest, %s radii of the real rows" % (count_r.shape, nearest2_r.shape, radius2_r.shape))
    if k < 1:
        raise ValueError("metrics: k %d (at least 1)" % k)
    if len(count_g) == 0 or len(count_r) == 0:
        return {m: float("nan") for m in METRICS}
    return dict(precision=float((count_g >= 1).mean()), recall=float((count_r >= 1).mean()),
                density=float(count_g.sum() / (float(k) * len(count_g))), coverage=float((nearest2_r <= radius2_r).mean()))


def summarise(count_g, count_r, nearest2_r, radius2_r, off_g, off_r, k, pooled):
    """Per-class metrics from vectors in class-grouped order (off_g / off_r [K + 1]: each class's row range) and the pooled ones from
    ``pooled`` = (count_g, count_r, nearest2_r, radius2_r) of the one-segment layout.  A class with <= k rows on either side is left
    out (nan); so is the pooled value when either whole set is that small."""
    K = len(off_g) - 1
    per = {m: np.full(K, np.nan) for m in METRICS}
    left = []
    for c in range(K):
        g, r = slice(off_g[c], off_g[c + 1]), slice(off_r[c], off_r[c + 1])
        if off_g[c + 1] - off_g[c] <= k or off_r[c + 1] - off_r[c] <= k:
            left.append(c)
            continue
        for m, v in metrics(count_g[g], count_r[r], nearest2_r[r], radius2_r[r], k).items():
            per[m][c] = v
    used = K - len(left)
    out = metrics(*pooled, k) if min(len(pooled[0]), len(pooled[1])) > k else {m: float("nan") for m in METRICS}
    for m in METRICS:
        out["intra_class_" + m] = float(np.nanmean(per[m])) if used else float("nan")
    out.update(per_class=per, left_out=left, classes_used=used)
    return out


# ------------------------------------------------------------------------------------------------------------- the two kernels
def knn_radius(ctx, x, off, k):
    """x: device tensor [n,d] fp32; off: device int32 [n_seg + 1].  -> device fp32 [n]: each row's squared distance to its k-th
    nearest other row of its segment (-1 in a segment of <= k rows).  One launch on ``ctx``'s stream, no synchronisation."""
    import torch
    check_rows(x, off, "knn_radius")
    with torch.cuda.stream(ctx.stream):
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    ctx.check(ctx.lib.rcgan_knn_radius(ctx.h, x.shape[0], x.shape[1], int(k), off.numel() - 1, C.c_void_p(x.data_ptr()),
                                       C.c_void_p(off.data_ptr()), C.c_void_p(out.data_ptr())))
    return out


def ball_query(ctx, q, q_off, r, r_off, r_radius2, want_count=True, want_nearest=True):
    """For every row of q: how many balls (r_j, r_radius2[j]) of its segment contain it, and the squared distance to the nearest r_j.
    -> (device int32 [nq] or None, device fp32 [nq] or None).  One launch on ``ctx``'s stream, no synchronisation."""
    import torch
    check_rows(q, q_off, "ball_query queries")
    check_rows(r, r_off, "ball_query references")
    if q.shape[1] != r.shape[1] or q_off.numel() != r_off.numel():
        raise ValueError("ball_query: queries %s / %d offsets, references %s / %d offsets" % (tuple(q.shape), q_off.numel(), tuple(r.shape), r_off.numel()))
    if want_count and (r_radius2 is None or r_radius2.dtype != torch.float32 or r_radius2.numel() != r.shape[0]):
        raise ValueError("ball_query: counting needs fp32 radii [%d]" % r.shape[0])
    with torch.cuda.stream(ctx.stream):
        count = torch.empty(q.shape[0], dtype=torch.int32, device=q.device) if want_count else None
        nearest = torch.empty(q.shape[0], dtype=torch.float32, device=q.device) if want_nearest else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ctx.check(ctx.lib.rcgan_ball_query(ctx.h, q.shape[0], r.shape[0], q.shape[1], q_off.numel() - 1, p(q), p(q_off), p(r), p(r_off),
                                       p(r_radius2), p(count), p(nearest)))
    return count, nearest


def radii(fs, k):
    """knn_radius on both layouts of a FeatureSet, kept on it as ``rad_pooled`` and ``rad_grouped``."""
    fs.rad_pooled = knn_radius(fs.ctx, fs.pooled, fs.d_off_pooled, k)
    fs.rad_grouped = knn_radius(fs.ctx, fs.grouped, fs.d_off_grouped, k)


def compare(real, generated, k):
    """real, generated: FeatureSet on the same context, ``radii(real, k)`` already taken.  -> the result dict of ``ManifoldEvaluator.evaluate``."""
    ctx = real.ctx
    if real.d != generated.d or len(real.count) != len(generated.count):
        raise ValueError("compare: real %d features x %d classes, generated %d x %d" % (real.d, len(real.count), generated.d, len(generated.count)))
    radii(generated, k)
    dev = []
    for R, Ro, Rr, G, Go, Gr in ((real.pooled, real.d_off_pooled, real.rad_pooled, generated.pooled, generated.d_off_pooled, generated.rad_pooled),
                                 (real.grouped, real.d_off_grouped, real.rad_grouped, generated.grouped, generated.d_off_grouped, generated.rad_grouped)):
        count_g, _ = ball_query(ctx, G, Go, R, Ro, Rr, want_nearest=False)          # real balls around the generated rows
        count_r, nearest_r = ball_query(ctx, R, Ro, G, Go, Gr)                       # generated balls around the real rows
        dev += [count_g, count_r, nearest_r, Rr]
    host = download(ctx, *dev)
    out = summarise(*host[4:], generated.off_grouped, real.off_grouped, k, tuple(host[:4]))
    out.update(rejected_real=real.rejected, rejected_generated=generated.rejected)
    return out


class ManifoldEvaluator(FeatureEvaluator):
    """The four metrics end to end for one run, in the shape of frechet.FrechetEvaluator: a LabelClassifier (its own unless ``clf``
    hands one over), the real set's features and radii taken once (``prepare_real``), then ``evaluate`` per generated set."""

    def __init__(self, n_classes, k=5, asset=None, device=0, chunk=1000, clf=None):
        if not 1 <= int(k) <= MAX_K or not 1 <= int(n_classes) <= MAX_SEGMENTS:
            raise ValueError("ManifoldEvaluator: k %d (1..%d), n_classes %d (1..%d)" % (k, MAX_K, n_classes, MAX_SEGMENTS))
        super().__init__(n_classes, asset, device, chunk, clf)
        self.k = int(k)

    def prepare_real(self, images, clean_labels, n_calibration=N_CALIBRATION):
        """images (the data set's CHW rows or NHWC) with their CLEAN labels.  Calibration on the first n_calibration images, as the
        Frechet evaluator's; a classifier handed over already calibrated keeps its calibration (both metrics read the same features)."""
        x = as_nhwc(images)
        self.calibrate(x, n_calibration)
        self.real = self.feature_set(x, clean_labels)
        radii(self.real, self.k)
        return self.real

    def evaluate(self, images, labels):
        """-> dict: pooled ``precision`` / ``recall`` / ``density`` / ``coverage``; ``intra_class_*`` (the mean over the classes that take
        part; nan if none does); ``per_class`` {metric: [K], nan where left out}; ``left_out`` (classes with <= k rows on either
        side); ``classes_used``; ``rejected_real`` / ``rejected_generated`` (rows whose label was outside [0, K), dropped)."""
        if self.real is None:
            raise RuntimeError("ManifoldEvaluator.evaluate needs prepare_real() first")
        return compare(self.real, self.feature_set(images, labels), self.k)


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = dict(result)
    out["per_class"] = {m: [nn(v) for v in result["per_class"][m]] for m in METRICS}
    for m in METRICS:
        out[m], out["intra_class_" + m] = nn(result[m]), nn(result["intra_class_" + m])
    out["left_out"] = [int(c) for c in result["left_out"]]
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set (its first 1000 images calibrate the features)"), ("generated", "the set to score")),
                      (("k", 5, "the k of the k-nearest-neighbour radii (1..16)"),),
                      lambda K, FLAGS, device: ManifoldEvaluator(K, k=FLAGS.k, asset=FLAGS.label_classifier, device=device), json_ready,
                      features=True)


if __name__ == '__main__':
    main()
