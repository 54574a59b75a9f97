"""Sliced Wasserstein distance on Laplacian-pyramid patch descriptors (SWD; Karras et al. 2018, section 5), pooled and per class:
how far is the distribution of generated class-c IMAGES from the distribution of real class-c images, and at which spatial scale?
It reads pixels, not the label classifier's features (frechet.py, manifold.py, kid.py), and unlike msssim.py (diversity inside the
generated set) and neighbours.py (memorisation) it compares the two distributions: the fine level sees texture, sharpness and noise,
the middle level shapes, the coarse level layout and colour; per class against the CLEAN real class it sees label mixing, which the
pooled value cannot.

Definition (restated in float64 by tests/swd_ref.py).  Three pyramid levels of an image, G0 = x, G1 = down(G0), G2 = down(G1),
  L0 = G0 - up(G1), L1 = G1 - up(G2), L2 = G2       (down: [1,4,6,4,1]/16 per axis, mirror boundary, even indices; up: zero-insert,
                                                    [1,4,6,4,1]/8 per axis);
a level's descriptors are its 7 x 7 x c neighbourhoods on a lattice of stride 4 / 2 / 1 (49 / 25 / 4 per 32 x 32 image, 36 / 16 / 1
per 28 x 28 image), normalised per image set (or class segment of it) and channel; with ``directions`` unit vectors w per level
(Gaussian, normalised in float64, cast to fp32, from a private RandomState) and m descriptors on each side
  SWD_l = 1e3 * mean over directions of mean_i |sort(A w)_i - sort(B w)_i|.
Equal counts are made by the evaluator: per class the first min(g_c, r_c) images of each side in the caller's order, pooled the first
min(n_g, n_r).  Beside every number stands its FLOOR, the same distance between two disjoint runs of the real set at the same
per-class count (rows [0, m') against [m', 2 m'), m' = min(g_c, r_c // 2)): the value depends on the sample size, the floor says
what "the same distribution" scores at that size.  Floors are computed on first need and kept per count vector.

csrc/swd.hip does the work: per level and side the channel moments of every segment (``swd_moments``), the projections of the
normalised descriptors (``swd_project``: one workgroup per image, the pyramid in LDS, +inf behind a segment's count), a bitonic
row sort (``sort_rows``) and the fp64 row sums of |a - b| (``absdiff_rowsum``).  Directions go through in chunks so that each of
the two projection buffers stays under BUFFER_BYTES (64 MiB; one direction at a time if a single one is larger).  Only the
[3, directions, segments] sums are downloaded; the means over them are float64 numpy.

Stand-alone:  python -m rcgan_amd.swd --real a.npz --generated b.npz [--n_classes K] [--directions 128]
(each file: ``images`` [n,32,32,3], [n,3072] CHW rows, [n,28,28,1] or [n,784] of raw pixels 0..255, ``labels`` [n]) prints the numbers
as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import download, standalone  # noqa: F401  (download: re-exported)
from .msssim import as_uint8_nhwc

LEVELS = 3
STRIDES = (4, 2, 1)
PATCH = 7
SIZES = (28, 32)                         # the kernel's heights and widths (include/rcgan_hip.h)
MAX_DIRECTIONS = 1024
BUFFER_BYTES = 64 << 20                  # the most one projection buffer takes
SEED = 0x5D15


def directions(n_dir, c, seed=SEED):
    """fp32 [3, n_dir, 49 c]: per level n_dir Gaussian vectors normalised in float64, then cast.  Private stream."""
    g = np.random.RandomState(seed).normal(size=(LEVELS, int(n_dir), PATCH * PATCH * int(c)))
    return (g / np.sqrt((g * g).sum(axis=2, keepdims=True))).astype(np.float32)


def positions(h, w, level):
    """Descriptors per image at a level."""
    return ((((h >> level) - PATCH) // STRIDES[level]) + 1) * ((((w >> level) - PATCH) // STRIDES[level]) + 1)


def as_images(images):
    x = as_uint8_nhwc(images)
    if x.shape[1] not in SIZES or x.shape[2] not in SIZES:
        raise ValueError("swd: images of %d x %d pixels, expected 28 or 32 a side" % (x.shape[1], x.shape[2]))
    return x


def pow2_at_least(v):
    return 1 << max(int(v) - 1, 0).bit_length()


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _check(what, t, dtype, dims):
    if t.dtype != dtype or t.dim() != dims or not t.is_contiguous():
        raise ValueError("%s: expected contiguous %s with %d dimensions, got %s %s" % (what, dtype, dims, tuple(t.shape), t.dtype))


def swd_moments(ctx, x, off, level):
    """x: device uint8 [n,h,w,c] sorted by segment; off: device int32 [n_seg + 1].  -> device fp64 [n_seg, c, 2]: sum and sum of
    squares of every channel over all descriptor entries of the segment.  Two launches on ``ctx``'s stream, no synchronisation."""
    import torch
    _check("swd_moments", x, torch.uint8, 4)
    _check("swd_moments offsets", off, torch.int32, 1)
    n, h, w, c = x.shape
    with torch.cuda.stream(ctx.stream):
        part = torch.empty((n, c, 2), dtype=torch.float64, device=x.device)
        mom = torch.empty((off.numel() - 1, c, 2), dtype=torch.float64, device=x.device)
    ctx.check(ctx.lib.rcgan_swd_moments(ctx.h, n, h, w, c, level, STRIDES[level], off.numel() - 1, C.c_void_p(x.data_ptr()),
                                        C.c_void_p(off.data_ptr()), C.c_void_p(part.data_ptr()), C.c_void_p(mom.data_ptr())))
    return mom


def swd_project(ctx, x, off, mom, dirs, level, width, out=None):
    """dirs: device fp32 [n_dir, 49 c].  -> device fp32 [n_dir, n_seg, width]: the projections of the normalised descriptors, +inf
    behind a segment's count (written into ``out``'s leading rows if given)."""
    import torch
    _check("swd_project", x, torch.uint8, 4)
    _check("swd_project offsets", off, torch.int32, 1)
    _check("swd_project moments", mom, torch.float64, 3)
    _check("swd_project directions", dirs, torch.float32, 2)
    n, h, w, c = x.shape
    n_seg, n_dir = off.numel() - 1, dirs.shape[0]
    if dirs.shape[1] != PATCH * PATCH * c or tuple(mom.shape) != (n_seg, c, 2):
        raise ValueError("swd_project: directions %s, moments %s for %d channels, %d segments" % (tuple(dirs.shape), tuple(mom.shape), c, n_seg))
    if out is None:
        with torch.cuda.stream(ctx.stream):
            out = torch.empty((n_dir, n_seg, width), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n_dir * n_seg * width:
        raise ValueError("swd_project: out %s %s too small for %d x %d x %d" % (tuple(out.shape), out.dtype, n_dir, n_seg, width))
    ctx.check(ctx.lib.rcgan_swd_project(ctx.h, n, h, w, c, level, STRIDES[level], n_seg, C.c_void_p(x.data_ptr()), C.c_void_p(off.data_ptr()),
                                        C.c_void_p(mom.data_ptr()), n_dir, C.c_void_p(dirs.data_ptr()), width, C.c_void_p(out.data_ptr())))
    return out


def sort_rows(ctx, x, rows, width):
    """Sorts the first rows * width floats of device fp32 tensor x as rows of ``width`` (a power of two), ascending, in place."""
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < rows * width:
        raise ValueError("sort_rows: expected contiguous fp32 of at least %d x %d, got %s %s" % (rows, width, tuple(x.shape), x.dtype))
    ctx.check(ctx.lib.rcgan_sort_rows_f32(ctx.h, rows, width, C.c_void_p(x.data_ptr())))
    return x


def absdiff_rowsum(ctx, a, b, count, rows, width, out):
    """out[r] (device fp64, at least ``rows``) = sum_{i < count[r mod n_seg]} |a[r][i] - b[r][i]|; count: device int32 [n_seg]."""
    import torch
    _check("absdiff_rowsum counts", count, torch.int32, 1)
    for t in (a, b):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < rows * width:
            raise ValueError("absdiff_rowsum: expected contiguous fp32 of at least %d x %d, got %s %s" % (rows, width, tuple(t.shape), t.dtype))
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < rows:
        raise ValueError("absdiff_rowsum: out %s %s, expected fp64 of at least %d" % (tuple(out.shape), out.dtype, rows))
    ctx.check(ctx.lib.rcgan_absdiff_rowsum(ctx.h, rows, width, count.numel(), C.c_void_p(count.data_ptr()), C.c_void_p(a.data_ptr()),
                                           C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr())))
    return out


def segment_sums(ctx, xa, xb, counts, dirs, buffer_bytes=BUFFER_BYTES):
    """xa, xb: device uint8 [N,h,w,c], each sorted by segment with ``counts`` [n_seg] (host) images per segment on BOTH sides;
    dirs: device fp32 [3, n_dir, 49 c].  -> device fp64 [3, n_dir, n_seg]: per level, direction and segment the sum over the
    segment's descriptors of |sort(A w)_i - sort(B w)_i|.  No synchronisation."""
    import torch
    counts = np.asarray(counts, np.int64)
    N, h, w, c = xa.shape
    if tuple(xb.shape) != tuple(xa.shape) or counts.sum() != N or N < 1:
        raise ValueError("segment_sums: sets %s and %s, %d images in the segments" % (tuple(xa.shape), tuple(xb.shape), counts.sum()))
    n_seg, n_dir = len(counts), dirs.shape[1]
    with torch.cuda.stream(ctx.stream):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(xa.device)
        sums = torch.empty((LEVELS, n_dir, n_seg), dtype=torch.float64, device=xa.device)
    for level in range(LEVELS):
        n_pos = positions(h, w, level)
        width = pow2_at_least(counts.max() * n_pos)
        chunk = int(max(1, min(n_dir, buffer_bytes // (n_seg * width * 4))))
        with torch.cuda.stream(ctx.stream):
            have = torch.from_numpy((counts * n_pos).astype(np.int32)).to(xa.device)
            pa = torch.empty((chunk, n_seg, width), dtype=torch.float32, device=xa.device)
            pb = torch.empty_like(pa)
        mom_a, mom_b = swd_moments(ctx, xa, off, level), swd_moments(ctx, xb, off, level)
        for d0 in range(0, n_dir, chunk):
            nd = min(chunk, n_dir - d0)
            for x, mom, p in ((xa, mom_a, pa), (xb, mom_b, pb)):
                swd_project(ctx, x, off, mom, dirs[level, d0:d0 + nd], level, width, out=p)
                sort_rows(ctx, p, nd * n_seg, width)
            absdiff_rowsum(ctx, pa, pb, have, nd * n_seg, width, sums[level, d0:d0 + nd])
    return sums


def distances(sums, counts, h, w):
    """The downloaded sums [3, n_dir, n_seg] -> float64 [n_seg, 3]: 1e3 * mean over directions and descriptors; nan for an empty segment."""
    counts = np.asarray(counts, np.float64)
    out = np.full((len(counts), LEVELS), np.nan)
    for level in range(LEVELS):
        m = counts * positions(h, w, level)
        out[counts > 0, level] = 1e3 * sums[level].mean(axis=0)[counts > 0] / m[counts > 0]
    return out


# ------------------------------------------------------------------------------------------------------------------ the evaluator
class ImageSet:
    """One image set on the device as uint8 NHWC: the rows whose label lies in [0, K) in the caller's order (pooled) and again sorted
    by class (stable: inside a class the caller's order holds), with the classes' counts."""

    def __init__(self, ctx, images, labels, n_classes):
        import torch
        x = as_images(images)
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        if len(lab) != len(x):
            raise ValueError("swd: %d images, %d labels" % (len(x), len(lab)))
        kept = np.flatnonzero((lab >= 0) & (lab < n_classes))
        self.rejected, self.n, self.shape = len(x) - len(kept), len(kept), x.shape[1:]
        self.rows = np.bincount(lab[kept], minlength=n_classes).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.rows)])[:-1]
        self.ctx = ctx
        with torch.cuda.stream(ctx.stream):
            self.pooled = torch.from_numpy(np.ascontiguousarray(x[kept])).to(ctx.device)
            order = torch.from_numpy(np.argsort(lab[kept], kind="stable")).to(ctx.device)
            self.sorted = self.pooled.index_select(0, order) if self.n else self.pooled

    def classes(self, take, skip=None):
        """Device rows: class by class rows [skip[c], skip[c] + take[c]) of the class."""
        import torch
        skip = np.zeros_like(take) if skip is None else skip
        rows = np.concatenate([self.start[c] + skip[c] + np.arange(take[c]) for c in range(len(take))]).astype(np.int64)
        with torch.cuda.stream(self.ctx.stream):
            return self.sorted.index_select(0, torch.from_numpy(rows).to(self.ctx.device))


def _summary(pooled, per, prefix=""):
    """pooled [3], per [K,3] (nan rows: classes not used) -> the keys of one side (the values or, with a prefix, the floors)."""
    used = ~np.isnan(per).any(axis=1)
    mean = per.mean(axis=1)
    nan = float("nan")
    return {prefix + "swd": float(pooled.mean()), prefix + "swd_levels": pooled,
            prefix + "intra_class_swd": float(mean[used].mean()) if used.any() else nan,
            prefix + "intra_class_swd_se": float(mean[used].std(ddof=1) / np.sqrt(used.sum())) if used.sum() >= 2 else nan,
            prefix + "intra_class_swd_levels": per[used].mean(axis=0) if used.any() else np.full(LEVELS, np.nan),
            prefix + "per_class": per}


class SwdEvaluator:
    """SWD end to end for one run: the real set uploaded once (``prepare_real``), then ``evaluate`` per generated set.  Owns a small
    runtime Context unless ``ctx`` hands one over."""

    def __init__(self, n_classes, directions=128, device=0, ctx=None, seed=SEED):
        if int(n_classes) < 1 or not (1 <= int(directions) <= MAX_DIRECTIONS):
            raise ValueError("SwdEvaluator: n_classes %d (at least 1), directions %d (1..%d)" % (n_classes, directions, MAX_DIRECTIONS))
        self.n_classes, self.directions, self.seed = int(n_classes), int(directions), int(seed)
        self.owns_ctx = ctx is None
        if ctx is None:
            from .runtime import Context
            ctx = Context(device, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
        self.ctx = ctx
        self.real = self.dirs = None
        self.floors = {}

    def prepare_real(self, images, clean_labels):
        """images (the data set's rows or NHWC) with their CLEAN labels."""
        import torch
        self.real = ImageSet(self.ctx, images, clean_labels, self.n_classes)
        if self.real.n < 2:
            raise ValueError("swd: %d real images with a label in [0, %d)" % (self.real.n, self.n_classes))
        self.host_dirs = directions(self.directions, self.real.shape[2], self.seed)
        with torch.cuda.stream(self.ctx.stream):
            self.dirs = torch.from_numpy(self.host_dirs).to(self.ctx.device)
        self.floors = {}
        return dict(images=self.real.n, rows=self.real.rows, rejected=self.real.rejected)

    def _queue(self, A, B, m_pooled, take, skip_b=None, pooled_b_from=0):
        """Queues the pooled and the per-class comparison of image sets A and B -> [(device sums or None, counts), ...]."""
        out = []
        if m_pooled >= 2:
            out.append((segment_sums(self.ctx, A.pooled[:m_pooled], B.pooled[pooled_b_from:pooled_b_from + m_pooled], [m_pooled], self.dirs), [m_pooled]))
        else:
            out.append((None, [0]))
        take = np.where(take >= 2, take, 0)
        if take.sum() > 0:
            out.append((segment_sums(self.ctx, A.classes(take), B.classes(take, skip_b), take, self.dirs), take))
        else:
            out.append((None, take))
        return out

    def _finish(self, queued):
        h, w, _ = self.real.shape
        tensors = [s for s, _ in queued if s is not None]
        host = download(self.ctx, *tensors) if tensors else []             # (one synchronisation for everything queued)
        host = iter([host] if len(tensors) == 1 else host)
        return [distances(next(host), counts, h, w) if s is not None else np.full((len(counts), LEVELS), np.nan) for s, counts in queued]

    def floor(self, g_rows, n_g):
        """The floor at the generated set's counts: two disjoint runs of the real set compared -> (pooled [3], per class [K,3])."""
        key = (int(n_g),) + tuple(int(v) for v in g_rows)
        if key not in self.floors:
            R = self.real
            half = np.minimum(g_rows, R.rows // 2)
            m = min(int(n_g), R.n // 2)
            pooled, per = self._finish(self._queue(R, R, m, half, skip_b=np.where(half >= 2, half, 0), pooled_b_from=m))
            self.floors[key] = (pooled[0], per)
        return self.floors[key]

    def evaluate(self, images, labels):
        """-> dict: ``swd`` (pooled, the mean over the three levels) and ``swd_levels`` [3]; ``per_class`` [K, 3] (nan where left
        out); ``intra_class_swd`` (the mean over the classes used of their level means), ``intra_class_swd_se`` (their standard
        deviation / sqrt(count); nan below 2), ``intra_class_swd_levels`` [3]; the same keys with the prefix ``floor_``: two disjoint
        runs of the real set at the same counts; ``images_used`` [K] (per side), ``classes_used``, ``left_out`` (classes with fewer
        than 2 images on either side); ``rejected_real`` / ``rejected_generated`` (rows whose label was outside [0, K), dropped)."""
        if self.real is None:
            raise RuntimeError("SwdEvaluator.evaluate needs prepare_real() first")
        R = self.real
        G = ImageSet(self.ctx, images, labels, self.n_classes)
        if G.shape != R.shape:
            raise ValueError("swd: generated images %s, real images %s" % (G.shape, R.shape))
        take = np.minimum(G.rows, R.rows)
        pooled, per = self._finish(self._queue(G, R, min(G.n, R.n), take))
        out = _summary(pooled[0], per)
        floor_pooled, floor_per = self.floor(G.rows, G.n)
        out.update(_summary(floor_pooled, floor_per, "floor_"))
        left = [int(c) for c in range(self.n_classes) if take[c] < 2]
        out.update(images_used=np.where(take >= 2, take, 0), classes_used=self.n_classes - len(left), left_out=left,
                   rejected_real=R.rejected, rejected_generated=G.rejected)
        return out

    def close(self):
        self.real = self.dirs = None
        if self.owns_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = dict(result)
    for prefix in ("", "floor_"):
        for key in ("swd", "intra_class_swd", "intra_class_swd_se"):
            out[prefix + key] = nn(result[prefix + key])
        for key in ("swd_levels", "intra_class_swd_levels"):
            out[prefix + key] = [nn(v) for v in result[prefix + key]]
        out[prefix + "per_class"] = [[nn(v) for v in row] for row in result[prefix + "per_class"]]
    out["images_used"] = [int(v) for v in result["images_used"]]
    out["left_out"] = [int(c) for c in result["left_out"]]
    for key in ("classes_used", "rejected_real", "rejected_generated"):
        out[key] = int(result[key])
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set"), ("generated", "the set to score")),
                      (("directions", 128, "directions per pyramid level (1..%d)" % MAX_DIRECTIONS),),
                      lambda K, FLAGS, device: SwdEvaluator(K, directions=FLAGS.directions, device=device), json_ready)


if __name__ == '__main__':
    main()
