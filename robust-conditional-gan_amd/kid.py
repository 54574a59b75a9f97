"""Kernel distance between two image sets, pooled and per class: the UNBIASED estimate of the squared maximum mean discrepancy under
the cubic polynomial kernel k(x, y) = (x.y / d + 1)^3 (the Kernel Inception Distance of Binkowski et al. 2018), on the 64-wide pooled
feature of the label classifier -- the feature the Frechet distance (frechet.py) and the k-NN metrics (manifold.py) read, under the
same calibration.  Where those two are biased by the sample size (a 64 x 64 covariance out of 100 rows per class; radii that shrink
with n), the expectation of this estimate between two samples of one distribution is 0 at every sample size, so a mean over 100
classes of 100 rows each can be compared across runs that differ in class count or sample count.

With g the generated rows and r the real rows of one segment (the whole set, one class against the real CLEAN class, or one subset),
m and n rows:
  KD = S_gg / (m (m-1)) + S_rr / (n (n-1)) - 2 S_gr / (m n)
  S_gg = sum_{i != j} k(g_i, g_j)      S_rr likewise      S_gr = sum_{i,j} k(g_i, r_j)
A segment with fewer than 2 rows on either side is left out (nan) and listed.  The value may be negative and is not clipped.

The pairwise part never exists as a matrix: csrc/ksum.hip computes, per row, the sum of the kernel over the reference rows of its
segment (``poly3_rowsum``: fp32 inner products on the matrix cores, everything after them fp64); only those vectors are downloaded
and everything after them (``unbiased_mmd2``, ``summarise``) is float64 numpy on the host.

The numbers are built around the engine's own small classifier: they are NOT comparable with published Inception KID values.

Stand-alone:  python -m rcgan_amd.kid --real a.npz --generated b.npz [--n_classes K] [--subset_size 1000] [--label_classifier asset]
(each file: ``images`` [n,32,32,3] or [n,3072] CHW rows of raw pixels 0..255, ``labels`` [n]) prints the same numbers as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import (N_CALIBRATION, FeatureEvaluator, FeatureSet, as_nhwc, check_rows, download, permuted_labels,  # noqa: F401
                         standalone)                    # (FeatureSet, as_nhwc, permuted_labels: re-exported for the callers of this module)
from .manifold import MAX_SEGMENTS

COEF0 = 1.0                              # with gamma = 1 / d: the kernel of the Kernel Inception Distance


def gamma_of(d):
    return 1.0 / d


def unbiased_mmd2(s_gg, s_rr, s_gr, m, n):
    """The estimate of one segment, float64.  s_gg, s_rr: kernel sums over the ordered pairs i != j WITHIN the generated / real rows;
    s_gr: the sum over all m n cross pairs.  nan with fewer than 2 rows on either side."""
    if m < 2 or n < 2:
        return float("nan")
    m, n = float(m), float(n)
    return float(np.float64(s_gg) / (m * (m - 1.0)) + np.float64(s_rr) / (n * (n - 1.0)) - 2.0 * np.float64(s_gr) / (m * n))


def _segment_values(gg, rr, gr, off_g, off_r):
    """unbiased_mmd2 of every segment out of row sums in segment order."""
    gg, rr, gr = (np.asarray(v, np.float64).reshape(-1) for v in (gg, rr, gr))
    if gg.shape != gr.shape:
        raise ValueError("kernel distance: %s self sums, %s cross sums of the generated rows" % (gg.shape, gr.shape))
    if len(off_g) != len(off_r) or off_g[-1] > len(gg) or off_r[-1] > len(rr):
        raise ValueError("kernel distance: offsets %s / %s for %d generated, %d real rows" % (list(off_g), list(off_r), len(gg), len(rr)))
    out = np.full(len(off_g) - 1, np.nan)
    for s in range(len(out)):
        g, r = slice(off_g[s], off_g[s + 1]), slice(off_r[s], off_r[s + 1])
        out[s] = unbiased_mmd2(gg[g].sum(), rr[r].sum(), gr[g].sum(), off_g[s + 1] - off_g[s], off_r[s + 1] - off_r[s])
    return out


def summarise(gg, rr, gr, off_g, off_r, pooled, blocks=None):
    """Per-class values from row sums in class-grouped order (gg [m]: each generated row's kernel sum over the OTHER generated rows of
    its class; rr [n] likewise for the real rows; gr [m]: over the real rows of its class; off_g / off_r [K + 1]: each class's row
    range), the full-sample value from ``pooled`` = (gg, rr, gr) of the one-segment layout, and mean and standard deviation over the
    subsets from ``blocks`` = (gg, rr, gr, block offsets [B + 1]) of the pooled rows cut into B contiguous subsets (None or B = 0:
    nan / 0).  A class with fewer than 2 rows on either side is left out (nan)."""
    per = _segment_values(gg, rr, gr, off_g, off_r)
    left = [int(c) for c in np.flatnonzero(np.isnan(per))]
    used = per[~np.isnan(per)]
    out = dict(kernel_distance=float(_segment_values(*pooled, [0, np.size(pooled[0])], [0, np.size(pooled[1])])[0]))
    out["intra_class_kernel_distance"] = float(used.mean()) if len(used) else float("nan")
    out["intra_class_kernel_distance_se"] = float(used.std(ddof=1) / np.sqrt(len(used))) if len(used) >= 2 else float("nan")
    subs = _segment_values(blocks[0], blocks[1], blocks[2], blocks[3], blocks[3]) if blocks is not None and len(blocks[3]) > 1 else np.zeros(0)
    out.update(subset_mean=float(subs.mean()) if len(subs) else float("nan"), subset_std=float(subs.std()) if len(subs) else float("nan"),
               subsets=len(subs), per_class=per, left_out=left, classes_used=len(used))
    return out


def block_offsets(m, n, subset_size):
    """Offsets [B + 1] of B = min(m, n) // subset_size contiguous subsets of subset_size rows (B = 0: [0]); at most MAX_SEGMENTS
    subsets, the kernel's bound on one call."""
    return np.arange(min(min(m, n) // subset_size, MAX_SEGMENTS) + 1, dtype=np.int64) * subset_size


# ------------------------------------------------------------------------------------------------------------------ the kernel
def poly3_rowsum(ctx, q, q_off, r, r_off, exclude_same_row=False):
    """q [nq,d], r [nr,d]: device fp32; q_off, r_off: device int32 [n_seg + 1].  -> device fp64 [nq]: for every row of q the sum of
    (<q_i, r_j> / d + 1)^3 over the rows j of r in its segment; exclude_same_row leaves out j == i (q and r the same tensor and
    offsets).  Rows in no segment are not written.  One launch on ``ctx``'s stream, no synchronisation."""
    import torch
    check_rows(q, q_off, "poly3_rowsum queries")
    check_rows(r, r_off, "poly3_rowsum references")
    if q.shape[1] != r.shape[1] or q_off.numel() != r_off.numel():
        raise ValueError("poly3_rowsum: queries %s / %d offsets, references %s / %d offsets" % (tuple(q.shape), q_off.numel(), tuple(r.shape), r_off.numel()))
    with torch.cuda.stream(ctx.stream):
        out = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(ctx.lib.rcgan_poly3_rowsum(ctx.h, q.shape[0], r.shape[0], q.shape[1], q_off.numel() - 1, p(q), p(q_off), p(r), p(r_off),
                                         gamma_of(q.shape[1]), COEF0, 1 if exclude_same_row else 0, p(out)))
    return out


def _device_offsets(ctx, off):
    import torch
    with torch.cuda.stream(ctx.stream):
        return torch.from_numpy(np.ascontiguousarray(off, np.int32)).to(ctx.device)


def self_sums(fs, block_off):
    """Device row sums of a FeatureSet against itself without the diagonal: [pooled, grouped, blocks or None]."""
    ctx = fs.ctx
    out = [poly3_rowsum(ctx, fs.pooled, fs.d_off_pooled, fs.pooled, fs.d_off_pooled, True),
           poly3_rowsum(ctx, fs.grouped, fs.d_off_grouped, fs.grouped, fs.d_off_grouped, True), None]
    if len(block_off) > 1:
        d_off = _device_offsets(ctx, block_off)
        out[2] = poly3_rowsum(ctx, fs.pooled, d_off, fs.pooled, d_off, True)
    return out


def compare(real, real_sums, generated, subset_size):
    """real, generated: FeatureSet on the same context; real_sums: the HOST vectors of ``self_sums(real, block_offsets(n, n,
    subset_size))``.  -> the result dict of ``KernelDistanceEvaluator.evaluate``.  Six launches and one download."""
    ctx = real.ctx
    if real.d != generated.d or len(real.count) != len(generated.count):
        raise ValueError("compare: real %d features x %d classes, generated %d x %d" % (real.d, len(real.count), generated.d, len(generated.count)))
    boff = block_offsets(generated.n, real.n, subset_size)
    dev = self_sums(generated, boff)
    dev += [poly3_rowsum(ctx, generated.pooled, generated.d_off_pooled, real.pooled, real.d_off_pooled),
            poly3_rowsum(ctx, generated.grouped, generated.d_off_grouped, real.grouped, real.d_off_grouped), None]
    if len(boff) > 1:
        d_off = _device_offsets(ctx, boff)
        dev[5] = poly3_rowsum(ctx, generated.pooled, d_off, real.pooled, d_off)
    have = [t for t in dev if t is not None]
    host = iter(download(ctx, *have))
    gg_p, gg_c, gg_b, gr_p, gr_c, gr_b = [next(host) if t is not None else None for t in dev]
    blocks = (gg_b, real_sums[2], gr_b, boff) if len(boff) > 1 else None
    out = summarise(gg_c, real_sums[1], gr_c, generated.off_grouped, real.off_grouped, (gg_p, real_sums[0], gr_p), blocks)
    out.update(rejected_real=real.rejected, rejected_generated=generated.rejected)
    return out


class KernelDistanceEvaluator(FeatureEvaluator):
    """The kernel distance end to end for one run, in the shape of manifold.ManifoldEvaluator: a LabelClassifier (its own unless
    ``clf`` hands one over), the real set's features and self row sums taken once (``prepare_real``), then ``evaluate`` per
    generated set."""

    def __init__(self, n_classes, subset_size=1000, asset=None, device=0, chunk=1000, clf=None):
        if not 1 <= int(n_classes) <= MAX_SEGMENTS or int(subset_size) < 2:
            raise ValueError("KernelDistanceEvaluator: n_classes %d (1..%d), subset_size %d (at least 2)" % (n_classes, MAX_SEGMENTS, subset_size))
        super().__init__(n_classes, asset, device, chunk, clf)
        self.subset_size = int(subset_size)
        self.real_sums = None

    def prepare_real(self, images, clean_labels, n_calibration=N_CALIBRATION):
        """images (the data set's CHW rows or NHWC) with their CLEAN labels.  Calibration on the first n_calibration images, as the
        Frechet evaluator's; a classifier handed over already calibrated keeps its calibration (all metrics read the same features)."""
        x = as_nhwc(images)
        self.calibrate(x, n_calibration)
        self.real = self.feature_set(x, clean_labels)
        dev = self_sums(self.real, block_offsets(self.real.n, self.real.n, self.subset_size))
        host = download(self.real.ctx, *[t for t in dev if t is not None])
        self.real_sums = host + [None] * (3 - len(host))
        return self.real

    def evaluate(self, images, labels):
        """-> dict: ``kernel_distance`` (the full-sample estimate); ``intra_class_kernel_distance`` (the mean over the classes that
        take part; nan if none does) and ``intra_class_kernel_distance_se`` (their standard deviation / sqrt(count); nan below 2);
        ``subset_mean`` / ``subset_std`` / ``subsets`` (the estimate on min(m, n) // subset_size contiguous subsets; nan / 0 without
        one); ``per_class`` [K], nan where left out; ``left_out`` (classes with < 2 rows on either side); ``classes_used``;
        ``rejected_real`` / ``rejected_generated`` (rows whose label was outside [0, K), dropped)."""
        if self.real is None:
            raise RuntimeError("KernelDistanceEvaluator.evaluate needs prepare_real() first")
        return compare(self.real, self.real_sums, self.feature_set(images, labels), self.subset_size)


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = dict(result)
    out["per_class"] = [nn(v) for v in result["per_class"]]
    for key in ("kernel_distance", "intra_class_kernel_distance", "intra_class_kernel_distance_se", "subset_mean", "subset_std"):
        out[key] = nn(result[key])
    out["left_out"] = [int(c) for c in result["left_out"]]
    out["subsets"], out["classes_used"] = int(result["subsets"]), int(result["classes_used"])
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set (its first 1000 images calibrate the features)"), ("generated", "the set to score")),
                      (("subset_size", 1000, "rows per subset of the mean +- std over subsets"),),
                      lambda K, FLAGS, device: KernelDistanceEvaluator(K, subset_size=FLAGS.subset_size, asset=FLAGS.label_classifier, device=device),
                      json_ready, features=True)


if __name__ == '__main__':
    main()
