"""Intra-class multi-scale structural similarity (MS-SSIM; Wang et al. 2003, used as a diversity measure by AC-GAN, Odena et al. 2017):
the similarity of random pairs of IMAGES of one class, class by class, beside the same number on the training data.  It reads pixels,
not the label classifier's features, so it sees what the Frechet distance (frechet.py), the k-NN metrics (manifold.py) and the kernel
distance (kid.py) cannot: a class whose generated pairs are more alike than its real pairs has lost modes; a class whose pairs are far
less alike than the real ones is probably a mixture of classes.

The value of a set of pairs is the reference's ``MultiScaleSSIM`` (cifar10/common/msssim.py) of the BATCH of those pairs: per scale
l = 0..4 the contrast-structure map's mean cs_l and the SSIM map's mean ssim_l are taken over all pairs, positions and channels, then
  MS-SSIM = prod_{l < 4} cs_l^{w_l} * ssim_4^{w_4},      w = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333.
Five scales on 32 x 32 images end in three scales whose map is a single position (the window shrinks to the 4 x 4, 2 x 2 and 1 x 1
levels), where the contrast-structure term of one pair of unrelated images is often negative and its fractional power undefined: that
is why the value is defined per class on batch means and not per pair.  A set whose mean is still not positive is nan ("undefined").

csrc/msssim.hip computes the ten per-scale means of every pair (``msssim_pairs``: one workgroup per pair, both images and all five
scales on chip); only that [P, 2, 5] array is downloaded and everything after it (``combine``, ``summarise``) is float64 numpy.

Stand-alone:  python -m rcgan_amd.msssim --real a.npz --generated b.npz [--n_classes K] [--pairs 1000]
(each file: ``images`` [n,32,32,3], [n,3072] CHW rows, [n,28,28,1] or [n,784] of raw pixels 0..255, ``labels`` [n]) prints the numbers
as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import download, standalone  # noqa: F401  (download: re-exported)

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
LEVELS = 5
MIN_HW, MAX_HW = 16, 32                  # the kernel's bounds on height and width (include/rcgan_hip.h)
SEED = 0x55104


def as_uint8_nhwc(images):
    """[n,3072] CHW rows (CIFAR's layout), [n,784] rows (MNIST's), [n,h,w] or [n,h,w,c] of raw pixels 0..255 -> uint8 [n,h,w,c]."""
    x = np.asarray(images)
    if x.ndim == 2 and x.shape[1] == 3072:
        x = x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    elif x.ndim == 2 and x.shape[1] == 784:
        x = x.reshape(-1, 28, 28, 1)
    elif x.ndim == 3:
        x = x[..., None]
    if x.ndim != 4 or x.shape[3] not in (1, 3) or not (MIN_HW <= x.shape[1] <= MAX_HW and MIN_HW <= x.shape[2] <= MAX_HW):
        raise ValueError("msssim: images %s, expected [n,h,w,c] with c 1 or 3 and %d <= h, w <= %d, [n,3072] or [n,784]"
                         % (np.shape(images), MIN_HW, MAX_HW))
    if x.dtype != np.uint8:
        if x.size and (x.min() < 0 or x.max() > 255):
            raise ValueError("msssim: pixels in [%s, %s], expected raw values 0..255" % (x.min(), x.max()))
        x = np.rint(x) if x.dtype.kind == "f" else x
    return np.ascontiguousarray(x, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the pairs
def _unrank(t):
    """Position t of the list (0,1), (0,2), (1,2), (0,3), ... of the unordered pairs i < j -> (i, j), int64 arrays."""
    t = np.asarray(t, np.int64)
    j = np.floor((1.0 + np.sqrt(1.0 + 8.0 * t.astype(np.float64))) / 2.0).astype(np.int64)
    j = np.where(j * (j - 1) // 2 > t, j - 1, j)                    # (the square root may be off by one either way)
    j = np.where(j * (j + 1) // 2 <= t, j + 1, j)
    return t - j * (j - 1) // 2, j


def _draw(rs, total, k):
    """min(k, total) distinct values of range(total): all of them in order if total <= k, else drawn from rs without replacement."""
    if total <= k:
        return np.arange(total, dtype=np.int64)
    if total <= 2 * k:
        return rs.permutation(total)[:k].astype(np.int64)
    got = np.zeros(0, np.int64)
    while len(got) < k:                                             # (at most half of range(total) is wanted: few rounds)
        both = np.concatenate([got, rs.randint(0, total, size=2 * (k - len(got)), dtype=np.int64)])
        _, first = np.unique(both, return_index=True)
        got = both[np.sort(first)][:k]
    return got


def class_pairs(labels, n_classes, pairs, seed):
    """The pairs one evaluation compares.  -> dict: ``pairs`` int32 [T, 2], row indices i < j into ``labels``; ``off`` int64 [K + 2]:
    class c's pairs are pairs[off[c]:off[c + 1]] -- min(pairs, n_c (n_c - 1) / 2) distinct unordered pairs of the class's rows, all of
    them if the class has no more, else drawn without replacement -- and pairs[off[K]:off[K + 1]] the pooled segment: ``pairs``
    distinct pairs (or all) over every accepted row, regardless of class; ``rows`` [K]: rows per class; ``rejected``: rows whose label
    is outside [0, K), dropped.  Drawn from a private RandomState(seed): deterministic, and the global numpy stream does not move."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    K, k = int(n_classes), int(pairs)
    if K < 1 or k < 1:
        raise ValueError("class_pairs: n_classes %d, pairs %d (at least 1 each)" % (K, k))
    rs = np.random.RandomState(seed)
    ok = (lab >= 0) & (lab < K)
    segments = [np.flatnonzero(lab == c) for c in range(K)] + [np.flatnonzero(ok)]
    out, off = [], [0]
    for rows in segments:
        i, j = _unrank(_draw(rs, len(rows) * (len(rows) - 1) // 2, k))
        out.append(np.stack([rows[i], rows[j]], axis=1))
        off.append(off[-1] + len(i))
    return dict(pairs=np.concatenate(out, axis=0).astype(np.int32).reshape(-1, 2), off=np.array(off, np.int64),
                rows=np.array([len(r) for r in segments[:K]], np.int64), rejected=int((~ok).sum()))


# ------------------------------------------------------------------------------------------------------------------ the host side
def combine(scales):
    """scales [P, 2, 5] (per pair: row 0 the contrast-structure mean, row 1 the SSIM mean of each scale) -> the MS-SSIM of the batch of
    those pairs, float64: the mean over the pairs per scale, then prod_{l<4} cs_l^{w_l} * ssim_4^{w_4}.  nan if a mean that enters a
    power is not positive (or there is no pair); nothing is clipped."""
    sc = np.asarray(scales, np.float64).reshape(-1, 2, LEVELS)
    if len(sc) == 0:
        return float("nan")
    m = sc.mean(axis=0)
    base = np.concatenate([m[0, :LEVELS - 1], m[1, LEVELS - 1:]])
    if not (base > 0).all():
        return float("nan")
    return float(np.prod(base ** WEIGHTS))


def summarise(scales, cp, real=None):
    """scales [T, 2, 5] of the pairs of ``cp`` (a class_pairs result); real: the result of this function on the real set, or None.
    -> the dict of ``MsssimEvaluator.evaluate`` (without the rejected counts; the ``real`` keys nan / 0 when real is None)."""
    sc = np.asarray(scales, np.float64).reshape(-1, 2, LEVELS)
    off, rows = cp["off"], cp["rows"]
    K = len(rows)
    if len(sc) != off[-1]:
        raise ValueError("summarise: %d rows of scales for %d pairs" % (len(sc), off[-1]))
    per, per_scales = np.full(K, np.nan), np.full((K, 2, LEVELS), np.nan)
    for c in range(K):
        if off[c + 1] > off[c]:
            per_scales[c] = sc[off[c]:off[c + 1]].mean(axis=0)
            per[c] = combine(sc[off[c]:off[c + 1]])
    left = [int(c) for c in range(K) if rows[c] < 2]
    used = per[~np.isnan(per)]
    real_per = np.full(K, np.nan) if real is None else np.asarray(real["per_class"], np.float64)
    both = ~np.isnan(per) & ~np.isnan(real_per)
    return dict(msssim=combine(sc[off[K]:off[K + 1]]),
                intra_class_msssim=float(used.mean()) if len(used) else float("nan"),
                intra_class_msssim_se=float(used.std(ddof=1) / np.sqrt(len(used))) if len(used) >= 2 else float("nan"),
                per_class=per, real_per_class=real_per,
                intra_class_msssim_real=float("nan") if real is None else real["intra_class_msssim"],
                msssim_real=float("nan") if real is None else real["msssim"],
                classes_above_real=int((per[both] > real_per[both]).sum()), classes_compared=int(both.sum()),
                per_class_scales=per_scales, pairs_used=(off[1:K + 1] - off[:K]).astype(np.int64), left_out=left,
                undefined=[int(c) for c in range(K) if rows[c] >= 2 and np.isnan(per[c])])


# ------------------------------------------------------------------------------------------------------------------ the kernel
def msssim_pairs(ctx, x, pairs):
    """x: device uint8 [n,h,w,c]; pairs: device int32 [P,2].  -> device fp32 [P,2,5]: per pair and scale the contrast-structure mean
    and the SSIM mean; nan for a pair with an index outside [0, n).  One launch on ``ctx``'s stream, no synchronisation."""
    import torch
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError("msssim_pairs: expected contiguous uint8 [n,h,w,c], got %s %s" % (tuple(x.shape), x.dtype))
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise ValueError("msssim_pairs: expected contiguous int32 [P,2], got %s %s" % (tuple(pairs.shape), pairs.dtype))
    with torch.cuda.stream(ctx.stream):
        out = torch.empty((pairs.shape[0], 2, LEVELS), dtype=torch.float32, device=x.device)
    n, h, w, c = x.shape
    ctx.check(ctx.lib.rcgan_msssim_pairs(ctx.h, n, h, w, c, pairs.shape[0], C.c_void_p(x.data_ptr()), C.c_void_p(pairs.data_ptr()),
                                         C.c_void_p(out.data_ptr())))
    return out


def upload(ctx, images, pairs):
    """uint8 [n,h,w,c] and int32 [P,2] host arrays -> their device tensors, copied on ``ctx``'s stream."""
    import torch
    with torch.cuda.stream(ctx.stream):
        return torch.from_numpy(images).to(ctx.device), torch.from_numpy(pairs).to(ctx.device)


class MsssimEvaluator:
    """Intra-class MS-SSIM end to end for one run: the real set's per-class and pooled values taken once (``prepare_real``), then
    ``evaluate`` per generated set.  Per image set: the images uploaded once as uint8, the pairs as one int32 array, one launch, one
    download.  Owns a small runtime Context unless ``ctx`` hands one over."""

    def __init__(self, n_classes, pairs=1000, seed=SEED, device=0, ctx=None):
        if int(n_classes) < 1 or int(pairs) < 1:
            raise ValueError("MsssimEvaluator: n_classes %d, pairs %d (at least 1 each)" % (n_classes, pairs))
        self.n_classes, self.pairs, self.seed = int(n_classes), int(pairs), int(seed)
        self.owns_ctx = ctx is None
        if ctx is None:
            from .runtime import Context
            ctx = Context(device, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
        self.ctx = ctx
        self.real = None

    def measure(self, images, labels):
        """-> (the class_pairs of the labels, float64 [T, 2, 5] per-scale means of those pairs)."""
        x = as_uint8_nhwc(images)
        if len(np.reshape(labels, -1)) != len(x):
            raise ValueError("msssim: %d images, %d labels" % (len(x), len(np.reshape(labels, -1))))
        cp = class_pairs(labels, self.n_classes, self.pairs, self.seed)
        if len(cp["pairs"]) == 0:
            return cp, np.zeros((0, 2, LEVELS))
        dx, dp = upload(self.ctx, x, cp["pairs"])
        return cp, download(self.ctx, msssim_pairs(self.ctx, dx, dp)).astype(np.float64)

    def prepare_real(self, images, clean_labels):
        """images (the data set's rows or NHWC) with their CLEAN labels."""
        cp, sc = self.measure(images, clean_labels)
        self.real = summarise(sc, cp)
        self.real["rejected"] = cp["rejected"]
        return self.real

    def evaluate(self, images, labels):
        """-> dict: ``msssim`` (the pooled pairs, regardless of class); ``intra_class_msssim`` (the mean over the classes whose value
        is defined; nan if none is) and ``intra_class_msssim_se`` (their standard deviation / sqrt(count); nan below 2); ``per_class``
        [K], nan where left out or undefined; ``real_per_class`` [K], ``intra_class_msssim_real`` and ``msssim_real`` (the same numbers
        of the real set); ``classes_above_real`` (classes, among the ``classes_compared`` defined on both sides, whose generated pairs
        are MORE alike than the real ones); ``per_class_scales`` [K, 2, 5] (the per-scale means behind per_class); ``pairs_used`` [K];
        ``left_out`` (classes with fewer than 2 rows); ``undefined`` (classes with a non-positive scale mean); ``rejected_real`` /
        ``rejected_generated`` (rows whose label was outside [0, K), dropped)."""
        if self.real is None:
            raise RuntimeError("MsssimEvaluator.evaluate needs prepare_real() first")
        cp, sc = self.measure(images, labels)
        out = summarise(sc, cp, self.real)
        out.update(rejected_real=self.real["rejected"], rejected_generated=cp["rejected"])
        return out

    def close(self):
        if self.owns_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = dict(result)
    for key in ("msssim", "intra_class_msssim", "intra_class_msssim_se", "intra_class_msssim_real", "msssim_real"):
        out[key] = nn(result[key])
    for key in ("per_class", "real_per_class"):
        out[key] = [nn(v) for v in result[key]]
    out["per_class_scales"] = [[[nn(v) for v in row] for row in cls] for cls in result["per_class_scales"]]
    out["pairs_used"] = [int(v) for v in result["pairs_used"]]
    for key in ("left_out", "undefined"):
        out[key] = [int(c) for c in result[key]]
    for key in ("classes_above_real", "classes_compared", "rejected_real", "rejected_generated"):
        if key in result:
            out[key] = int(result[key])
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set"), ("generated", "the set to score")),
                      (("pairs", 1000, "pairs per class (and of the pooled value)"), ("seed", SEED, "seed of the pair draw")),
                      lambda K, FLAGS, device: MsssimEvaluator(K, pairs=FLAGS.pairs, seed=FLAGS.seed, device=device), json_ready)


if __name__ == '__main__':
    main()
