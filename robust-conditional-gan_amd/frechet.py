"""Frechet distance between two image sets, pooled and per class, on the 64-wide pooled feature of the label classifier
(eval_cifar.LabelClassifier: the pre-activation ResNet-32 on the engine's fp32 kernels).

Features come from the classifier's FROZEN pass (``LabelClassifier.calibrate`` once on real images, then ``features``): a sample's
feature does not depend on its batch.  The device accumulates count, sum x and sum x x^T per class in fp64 (csrc/moments.hip,
``ClassMoments``); everything after that -- means, covariances, the pooled moments (the per-class sums added up, not a second
kernel) and the distance -- is float64 numpy on the host.

The number is built around the engine's own small classifier: it is NOT comparable with published Inception-v3 FID values.

Stand-alone:  python -m rcgan_amd.frechet --real a.npz --generated b.npz   (each file: ``images`` [n,32,32,3] or [n,3072] CHW
rows of raw pixels 0..255, ``labels`` [n]) prints the same numbers as one JSON line."""
import collections
import ctypes as C
import hashlib
import json
import os
import zipfile

import numpy as np

from . import _lib as L
from .evaluators import N_CALIBRATION, FeatureEvaluator, as_nhwc, permuted_labels, standalone  # noqa: F401  (permuted_labels: re-exported)

CACHE_NAME = "frechet_real_stats.npz"

# count [K], mean [K,d], cov [K,d,d] (unbiased, n - 1; zeros for a class with fewer than 2 rows), pooled = (n, mean [d], cov [d,d]) of
# all accepted rows, rejected = rows whose label was outside [0, K); float64
Moments = collections.namedtuple("Moments", "count mean cov pooled rejected")


def _mean_cov(n, s, ss):
    """(n, sum x [d], sum x x^T [d,d]) -> (mean, unbiased covariance), float64.  Fewer than 2 rows: a zero covariance."""
    d = s.shape[0]
    if n < 1:
        return np.zeros(d), np.zeros((d, d))
    m = s / n
    if n < 2:
        return m, np.zeros((d, d))
    c = (ss - n * np.outer(m, m)) / (n - 1.0)
    return m, 0.5 * (c + c.T)


def moments_from_sums(count, sums, sumsq, rejected=0):
    """The kernel's state (count [K], sum [K,d], sumsq [K,d,d]) -> Moments.  The pooled triple is formed from the per-class sums."""
    count = np.asarray(count, np.float64)
    sums, sumsq = np.asarray(sums, np.float64), np.asarray(sumsq, np.float64)
    K, d = sums.shape
    mean, cov = np.zeros((K, d)), np.zeros((K, d, d))
    for k in range(K):
        mean[k], cov[k] = _mean_cov(count[k], sums[k], sumsq[k])
    n = float(count.sum())
    pm, pc = _mean_cov(n, sums.sum(0), sumsq.sum(0))
    return Moments(count, mean, cov, (n, pm, pc), int(rejected))


def moments_of(features, labels, n_classes):
    """Host restatement of the device accumulation (float64 sums of the same products): features [n,d], labels [n] or None."""
    x = np.asarray(features, np.float64)
    n, d = x.shape
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels).reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < n_classes)
    count, sums, sumsq = np.zeros(n_classes), np.zeros((n_classes, d)), np.zeros((n_classes, d, d))
    for k in np.unique(lab[ok]):
        xs = x[lab == k]
        count[k], sums[k], sumsq[k] = len(xs), xs.sum(0), xs.T.dot(xs)
    return moments_from_sums(count, sums, sumsq, int((~ok).sum()))


class ClassMoments:
    """Device state of rcgan_class_moments_accum for d-wide features and K classes on ``ctx``'s stream: allocated and zeroed here,
    ``add`` per batch (one launch, no synchronisation), one ``download`` at the end."""

    def __init__(self, ctx, d, n_classes):
        import torch
        self.ctx, self.d, self.n_classes = ctx, int(d), int(n_classes)
        nbytes = ctx.lib.rcgan_class_moments_bytes(self.d, self.n_classes)
        if nbytes == 0:
            raise ValueError("ClassMoments: d %d (1..256), n_classes %d (1..%d)" % (d, n_classes, L.MAX_CLASSES))
        with torch.cuda.stream(ctx.stream):
            self.state = torch.zeros(nbytes // 8, dtype=torch.float64, device=ctx.device)

    def add(self, feat, labels=None):
        """feat: device tensor [n,d] fp32; labels: int32 device tensor [n], or None (one class only)."""
        ctx = self.ctx
        if feat.dtype != L.F32 or len(feat.shape) != 2 or feat.shape[1] != self.d:
            raise ValueError("features %s dtype %s: expected fp32 [n,%d]" % (feat.shape, feat.dtype, self.d))
        if labels is not None and (labels.dtype != "i32" or labels.size != feat.shape[0]):
            raise ValueError("labels: expected int32 [%d]" % feat.shape[0])
        ctx.check(ctx.lib.rcgan_class_moments_accum(ctx.h, feat.shape[0], self.d, self.n_classes, C.c_void_p(feat.ptr),
                                                    C.c_void_p(labels.ptr) if labels is not None else None,
                                                    C.c_void_p(self.state.data_ptr())))

    def zero(self):
        import torch
        with torch.cuda.stream(self.ctx.stream):
            self.state.zero_()

    def download_state(self):
        """-> (count [K], sum [K,d], sumsq [K,d,d], rejected) float64, as the kernel holds them."""
        import torch
        K, d = self.n_classes, self.d
        with torch.cuda.stream(self.ctx.stream):
            host = self.state.cpu()
        self.ctx.stream.synchronize()
        a = host.numpy()
        return a[:K].copy(), a[K:K + K * d].reshape(K, d).copy(), a[K + K * d:K + K * d + K * d * d].reshape(K, d, d).copy(), int(a[-1])

    def download(self):
        return moments_from_sums(*self.download_state())


def frechet_distance(m1, S1, m2, S2):
    """|m1 - m2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 in float64.  The trace term is the sum of the square roots of the eigenvalues
    of S1^1/2 S2 S1^1/2 (symmetric, so ``eigh``; S1^1/2 from ``eigh`` too), negative eigenvalues clipped to 0: rank-deficient
    covariances give a finite, non-negative number."""
    m1, m2 = np.asarray(m1, np.float64).reshape(-1), np.asarray(m2, np.float64).reshape(-1)
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    d = m1.shape[0]
    if m2.shape != (d,) or S1.shape != (d, d) or S2.shape != (d, d):
        raise ValueError("frechet_distance: shapes %s %s %s %s" % (m1.shape, S1.shape, m2.shape, S2.shape))
    S1, S2 = 0.5 * (S1 + S1.T), 0.5 * (S2 + S2.T)
    w, v = np.linalg.eigh(S1)
    root = (v * np.sqrt(np.clip(w, 0.0, None))).dot(v.T)
    mid = root.dot(S2).dot(root)
    ev = np.linalg.eigvalsh(0.5 * (mid + mid.T))
    tr = float(np.sqrt(np.clip(ev, 0.0, None)).sum())
    diff = m1 - m2
    return max(float(diff.dot(diff) + np.trace(S1) + np.trace(S2) - 2.0 * tr), 0.0)


def evaluate(real, generated, min_count=2):
    """real, generated: Moments over the same classes and feature width.  -> dict: ``frechet_distance`` (pooled),
    ``intra_class_frechet_distance`` (mean of the per-class distances over the classes that take part; nan if none does),
    ``per_class`` (nan where left out), ``left_out`` (classes with fewer than min_count samples on either side), ``classes_used``,
    ``rejected_real`` / ``rejected_generated`` (rows whose label was outside [0, K))."""
    K = len(real.count)
    if len(generated.count) != K or real.mean.shape != generated.mean.shape:
        raise ValueError("evaluate: %s real classes x features, %s generated" % (real.mean.shape, generated.mean.shape))
    per, left = np.full(K, np.nan), []
    for k in range(K):
        if real.count[k] < min_count or generated.count[k] < min_count:
            left.append(k)
        else:
            per[k] = frechet_distance(real.mean[k], real.cov[k], generated.mean[k], generated.cov[k])
    used = K - len(left)
    pooled = frechet_distance(real.pooled[1], real.pooled[2], generated.pooled[1], generated.pooled[2]) \
        if min(real.pooled[0], generated.pooled[0]) >= min_count else float("nan")
    return dict(frechet_distance=pooled, intra_class_frechet_distance=float(np.nanmean(per)) if used else float("nan"),
                per_class=per, left_out=left, classes_used=used, rejected_real=real.rejected, rejected_generated=generated.rejected)


# --------------------------------------------------------------------------------------------------------- the real set's cache
def file_sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def array_sha256(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def real_statistics(path, key, compute):
    """The real set's moments and the calibration pairs, from ``path`` when the file was written under the same ``key`` (a dict of
    strings / integers: the classifier asset's SHA-256, the number of real images, a hash of the calibration images ...), else from
    ``compute()`` -> (Moments, {layer: (mean, variance)}) and written there.  -> (Moments, pairs, reused)."""
    want = json.dumps(key, sort_keys=True)
    if path is not None and os.path.exists(path):
        try:
            with np.load(path, allow_pickle=False) as z:
                if str(z["key"]) == want:
                    names = json.loads(str(z["layers"]))
                    pairs = {k: (z["calib_mean_%d" % i], z["calib_var_%d" % i]) for i, k in enumerate(names)}
                    mom = Moments(z["count"], z["mean"], z["cov"], (float(z["pooled_n"]), z["pooled_mean"], z["pooled_cov"]), int(z["rejected"]))
                    return mom, pairs, True
        except (OSError, KeyError, ValueError, zipfile.BadZipFile):
            pass                        # unreadable or from another layout: recompute and overwrite
    mom, pairs = compute()
    if path is not None:
        names = sorted(pairs)
        arrays = dict(key=np.array(want), layers=np.array(json.dumps(names)), count=mom.count, mean=mom.mean, cov=mom.cov,
                      pooled_n=np.float64(mom.pooled[0]), pooled_mean=mom.pooled[1], pooled_cov=mom.pooled[2], rejected=np.int64(mom.rejected))
        for i, k in enumerate(names):
            arrays["calib_mean_%d" % i], arrays["calib_var_%d" % i] = np.asarray(pairs[k][0], np.float32), np.asarray(pairs[k][1], np.float32)
        tmp = path + ".tmp.npz"
        np.savez(tmp, **arrays)
        os.replace(tmp, path)
    return mom, pairs, False


class FrechetEvaluator(FeatureEvaluator):
    """The metric end to end for one run: a LabelClassifier (its own unless ``clf`` hands one over), the real set's statistics taken
    once (``prepare_real``, which always sets the classifier's calibration: computed here or restored from the cache), then
    ``evaluate`` per generated set."""

    def __init__(self, n_classes, asset=None, device=0, chunk=1000, clf=None):
        super().__init__(n_classes, asset, device, chunk, clf)
        self.reused = False

    def moments(self, images, labels):
        """Moments of the frozen features of ``images`` (NHWC) per class of ``labels``: chunks through the device kernel, one download."""
        mom = ClassMoments(self.clf.ctx, self.clf.FEATURE_DIM, self.n_classes)
        self.clf.features(images, labels, moments=mom, chunk=self.chunk)
        return mom.download()

    def prepare_real(self, images, labels, cache_path=None, n_calibration=N_CALIBRATION):
        """images (the data set's CHW rows or NHWC) with their CLEAN labels.  Calibration on the first n_calibration images."""
        x = as_nhwc(images)
        calib = x[:n_calibration]
        key = dict(asset_sha256=file_sha256(self.asset), n_real=int(len(x)), n_classes=self.n_classes,
                   calibration_sha256=array_sha256(np.asarray(calib, np.float32)))

        def compute():
            self.clf.calibrate(calib)
            return self.moments(x, labels), self.clf.calibration()
        self.real, pairs, self.reused = real_statistics(cache_path, key, compute)
        if self.reused:
            self.clf.set_calibration(pairs)
        return self.real

    def evaluate(self, images, labels, min_count=2):
        if self.real is None:
            raise RuntimeError("FrechetEvaluator.evaluate needs prepare_real() first")
        return evaluate(self.real, self.moments(as_nhwc(images), labels), min_count)


def json_ready(result):
    out = dict(result)
    out["per_class"] = [None if np.isnan(v) else float(v) for v in result["per_class"]]
    for k in ("frechet_distance", "intra_class_frechet_distance"):
        out[k] = None if np.isnan(result[k]) else float(result[k])
    out["left_out"] = [int(k) for k in result["left_out"]]
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set (its first 1000 images calibrate the features)"), ("generated", "the set to score")),
                      (("min_count", 2, "classes with fewer samples on either side are left out"),),
                      lambda K, FLAGS, device: FrechetEvaluator(K, asset=FLAGS.label_classifier, device=device), json_ready, features=True,
                      evaluate=lambda ev, FLAGS, x, y: ev.evaluate(x, y, FLAGS.min_count))


if __name__ == '__main__':
    main()
