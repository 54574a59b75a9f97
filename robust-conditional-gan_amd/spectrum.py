"""Radial power-spectrum distance of generated images, pooled and per class: do the generated class-c IMAGES carry their energy at the
same spatial frequencies as the real class-c images?  The other pixel metrics (msssim.py, neighbours.py, swd.py) look at images in
the spatial domain; the known failures of an upsampling generator are easiest to see in the frequency domain: excess energy at the
Nyquist frequencies (stripes at (N/2, 0) and (0, N/2), a checkerboard at (N/2, N/2)) and too little high-frequency energy over-all
(Durall et al. 2020; Dzanic et al. 2020; Schwarz et al. 2021).

Definition (restated in float64 by tests/spectrum_ref.py).  Images are uint8 NHWC, square, N a side (8..32), c 1 or 3.
  a = x - 128,  F_ch(u,v) = sum_{y,x} a[y,x,ch] exp(-2 pi i (u y + v x) / N),  P = |F|^2 / N^2;
  f(u) = u if u <= N // 2 else u - N;  the ring of (u,v) is the integer b with (2b - 1)^2 <= 4 (f(u)^2 + f(v)^2) < (2b + 1)^2 (ring 0
  is the point (0,0) alone; integers only);  B(N) = 1 + the largest ring;  S[i][ch][b] = the mean of P over the members of ring b.
A segment is the pooled set or one class; Sbar[ch][b] is the fp64 mean of S over its images.  Between a generated segment g and a
real segment r, with D[ch][b] = 10 log10(Sbar_g / Sbar_r) dB:
  spectral_distance  = sqrt(mean over ch and b = 1..B-1 of D^2)         (log-spectral distance; ring 0 is brightness and stays out)
  high_frequency_db  = 10 log10(HF_g / HF_r),  HF = sum_ch sum_{b > N/4} count_b Sbar / sum_ch sum_{b >= 1} count_b Sbar
  nyquist_db         = mean over ch of D[ch][N/2]     (the axis Nyquist ring: stripes; even N only)
  checkerboard_db    = mean over ch of D[ch][B-1]     (the ring of (N/2, N/2), at 28 and 32 that point alone; even N only)
A ring whose mean is 0 on either side is dropped from the segment's means; a segment with no ring left is undefined (listed, not
averaged); a class with fewer than 2 images on either side is left out (listed).  Beside the distance stands its FLOOR, the same number
between two disjoint runs of the real set: per class rows [0, m') against [m', 2 m'), m' = min(g_c, r_c // 2), pooled the first
min(n_g, n_r // 2) against the next as many, in the caller's order.  Floors are computed on first need and kept per count vector.

csrc/spectrum.hip computes S (``radial_spectrum``: one launch, one workgroup per image at a time, the transform as six N x N x N real
products per channel); the segment sums come from rcgan_class_moments_accum over the [n, c B] rows (``class_sums``: a label outside
[0, K) is skipped by that call, which is how a row range is selected for the floors).  Only the counts and sums are downloaded; the
means and logarithms are float64 numpy.

Stand-alone:  python -m rcgan_amd.spectrum --real a.npz --generated b.npz [--n_classes K]
(each file: ``images`` [n,32,32,3], [n,3072] CHW rows, [n,28,28,1] or [n,784] of raw pixels 0..255, ``labels`` [n]) prints the numbers
as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import download, standalone
from .msssim import as_uint8_nhwc

MIN_SIDE, MAX_SIDE = 8, 32               # the kernel's sizes (include/rcgan_hip.h)
DB_NAMES = ("high_frequency_db", "nyquist_db", "checkerboard_db")


def rings(N):
    """-> (int table [N,N]: the ring of every (u,v), int counts [B(N)]: the rings' members).  Integer arithmetic only."""
    N = int(N)
    f = np.arange(N)
    f = np.where(f <= N // 2, f, f - N)
    r2 = 4 * (f[:, None] ** 2 + f[None, :] ** 2)
    table = np.zeros((N, N), np.int64)
    b = 0
    while ((2 * b + 1) ** 2 <= r2).any():
        table += (2 * b + 1) ** 2 <= r2
        b += 1
    return table, np.bincount(table.reshape(-1))


def as_images(images):
    x = as_uint8_nhwc(images)
    if x.ndim != 4 or x.shape[1] != x.shape[2] or not (MIN_SIDE <= x.shape[1] <= MAX_SIDE) or x.shape[3] not in (1, 3):
        raise ValueError("spectrum: images %s, expected [n,N,N,c] with %d <= N <= %d and c 1 or 3" % (x.shape, MIN_SIDE, MAX_SIDE))
    return x


# ------------------------------------------------------------------------------------------------------------------ the device calls
def radial_spectrum(ctx, x, out=None):
    """x: device uint8 [n,N,N,c] -> device fp32 [n, c, B(N)] (written into ``out`` if given).  One launch on ``ctx``'s stream."""
    import torch
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous() or x.shape[1] != x.shape[2] or x.shape[0] < 1:
        raise ValueError("radial_spectrum: expected contiguous uint8 [n,N,N,c], got %s %s" % (tuple(x.shape), x.dtype))
    n, N, _, c = x.shape
    if not (MIN_SIDE <= N <= MAX_SIDE) or c not in (1, 3):
        raise ValueError("radial_spectrum: N %d (%d..%d), c %d (1 or 3)" % (N, MIN_SIDE, MAX_SIDE, c))
    B = len(rings(N)[1])
    if out is None:
        with torch.cuda.stream(ctx.stream):
            out = torch.empty((n, c, B), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, c, B):
        raise ValueError("radial_spectrum: out %s %s, expected fp32 %s" % (tuple(out.shape), out.dtype, (n, c, B)))
    ctx.check(ctx.lib.rcgan_radial_spectrum(ctx.h, n, N, c, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())))
    return out


def image_spectra(ctx, x):
    """Host uint8 [n,N,N,c] -> the images' reduced spectra as device fp32 rows [n, c B]: the upload and the kernel, no synchronisation."""
    import torch
    with torch.cuda.stream(ctx.stream):
        dx = torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
    return radial_spectrum(ctx, dx).reshape(len(x), -1)


def class_sums(ctx, rows, labels, n_classes):
    """rows: what ``image_spectra`` gave, [n,d]; labels: host int [n] -> float64 (count [K], sum [K,d]) over the rows of every label in
    [0, K); any other label's row is skipped.  One launch of rcgan_class_moments_accum and one download of the counts and sums."""
    import torch
    n, d = rows.shape
    nbytes = ctx.lib.rcgan_class_moments_bytes(d, n_classes)
    if nbytes == 0 or len(labels) != n:
        raise ValueError("class_sums: rows %s, %d labels, %d classes" % (tuple(rows.shape), len(labels), n_classes))
    with torch.cuda.stream(ctx.stream):
        lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(ctx.device)
        state = torch.zeros(nbytes // 8, dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.lib.rcgan_class_moments_accum(ctx.h, n, d, n_classes, C.c_void_p(rows.data_ptr()), C.c_void_p(lab.data_ptr()),
                                                C.c_void_p(state.data_ptr())))
    head = download(ctx, state[:n_classes * (1 + d)])
    return head[:n_classes].copy(), head[n_classes:].reshape(n_classes, d).copy()


# ------------------------------------------------------------------------------------------------------------------ the host arithmetic
def compare(g, r, counts, N):
    """g, r: float64 segment means [c, B]; counts: the rings' members [B] -> the four numbers of the segment pair (nan: undefined)."""
    nan = float("nan")
    B = g.shape[1]
    ok = (g > 0) & (r > 0)
    D = np.full(g.shape, np.nan)
    D[ok] = 10.0 * np.log10(g[ok] / r[ok])
    out = dict(spectral_distance=float(np.sqrt(np.mean(D[:, 1:][ok[:, 1:]] ** 2))) if ok[:, 1:].any() else nan)
    high = np.arange(B) > N // 4
    hf = [float((s[:, high] * counts[high]).sum() / (s[:, 1:] * counts[1:]).sum()) if (s[:, 1:] * counts[1:]).sum() > 0 else 0.0 for s in (g, r)]
    out["high_frequency_db"] = float(10.0 * np.log10(hf[0] / hf[1])) if hf[0] > 0 and hf[1] > 0 else nan
    for name, b in (("nyquist_db", N // 2), ("checkerboard_db", B - 1)):
        out[name] = float(D[ok[:, b], b].mean()) if N % 2 == 0 and ok[:, b].any() else nan
    return out


def _mean(count, total):
    """Segment means from counts [K] and sums [K,d]; nan rows where a segment is empty."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count[:, None] > 0, total / count[:, None], np.nan)


def _nanmean(v):
    v = np.asarray(v, np.float64)
    return float(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else float("nan")


class SpectrumEvaluator:
    """The spectral numbers end to end for one run: the real set's spectra once (``prepare_real``), then ``evaluate`` per generated
    set.  Owns a small runtime Context unless ``ctx`` hands one over."""

    def __init__(self, n_classes, device=0, ctx=None):
        if int(n_classes) < 1:
            raise ValueError("SpectrumEvaluator: n_classes %d (at least 1)" % n_classes)
        self.n_classes = int(n_classes)
        self.owns_ctx = ctx is None
        if ctx is None:
            from .runtime import Context
            ctx = Context(device, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
        self.ctx = ctx
        self.real = self.last = None
        self.floors = {}

    def _set(self, images, labels):
        """-> dict: the kept rows' spectra, labels, per-class counts and float64 means [K,c,B], the pooled mean [c,B]."""
        x = as_images(images)
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        if len(lab) != len(x):
            raise ValueError("spectrum: %d images, %d labels" % (len(x), len(lab)))
        kept = (lab >= 0) & (lab < self.n_classes)
        s = dict(rejected=int((~kept).sum()), n=int(kept.sum()), shape=x.shape[1:], labels=lab[kept])
        if s["n"] < 1:
            raise ValueError("spectrum: no image has a label in [0, %d)" % self.n_classes)
        s["rows"] = image_spectra(self.ctx, x[kept])
        count, total = class_sums(self.ctx, s["rows"], s["labels"], self.n_classes)
        c = x.shape[3]
        s["count"] = count.astype(np.int64)
        s["per_class"] = _mean(count, total).reshape(self.n_classes, c, -1)
        s["pooled"] = (total.sum(axis=0) / count.sum()).reshape(c, -1)
        return s

    def prepare_real(self, images, clean_labels):
        """images (the data set's rows or NHWC) with their CLEAN labels."""
        self.real = self._set(images, clean_labels)
        if self.real["n"] < 2:
            raise ValueError("spectrum: %d real images with a label in [0, %d)" % (self.real["n"], self.n_classes))
        self.side = self.real["shape"][0]
        self.ring_counts = rings(self.side)[1].astype(np.float64)
        self.floors, self.last = {}, None
        return dict(images=self.real["n"], rows=self.real["count"], rejected=self.real["rejected"])

    def _compare(self, g, r):
        return compare(g, r, self.ring_counts, self.side)

    def floor(self, g_rows, n_g):
        """The floor at the generated set's counts: two disjoint runs of the real set -> (pooled distance, per class [K])."""
        key = (int(n_g),) + tuple(int(v) for v in g_rows)
        if key not in self.floors:
            R, K = self.real, self.n_classes
            c = R["shape"][2]
            m = min(int(n_g), R["n"] // 2)
            pooled = float("nan")
            if m >= 2:
                run = np.full(R["n"], -1, np.int64)
                run[:m], run[m:2 * m] = 0, 1
                count, total = class_sums(self.ctx, R["rows"], run, 2)
                mean = _mean(count, total).reshape(2, c, -1)
                pooled = self._compare(mean[0], mean[1])["spectral_distance"]
            half = np.minimum(np.asarray(g_rows, np.int64), R["count"] // 2)
            half = np.where(half >= 2, half, 0)
            per = np.full(K, np.nan)
            if half.sum() > 0:
                rank = np.zeros(R["n"], np.int64)                      # a row's place inside its class, in the caller's order
                order = np.argsort(R["labels"], kind="stable")
                start = np.concatenate([[0], np.cumsum(R["count"])])[:-1]
                rank[order] = np.arange(R["n"]) - start[R["labels"][order]]
                h = half[R["labels"]]
                means = []
                for lo in (0, 1):                                      # the first run, then the second: one call each, K classes
                    run = np.where((rank >= lo * h) & (rank < (lo + 1) * h), R["labels"], -1)
                    means.append(_mean(*class_sums(self.ctx, R["rows"], run, K)).reshape(K, c, -1))
                for k in np.flatnonzero(half):
                    per[k] = self._compare(means[0][k], means[1][k])["spectral_distance"]
            self.floors[key] = (pooled, per)
        return self.floors[key]

    def evaluate(self, images, labels):
        """-> dict: ``spectral_distance``, ``high_frequency_db``, ``nyquist_db``, ``checkerboard_db`` (pooled); the same four with the
        prefix ``per_class_`` ([K], nan where left out or undefined) and ``intra_class_`` (their means over the classes that have
        one), ``intra_class_spectral_distance_se`` (standard deviation / sqrt(count); nan below 2); ``floor_spectral_distance``,
        ``floor_per_class_spectral_distance``, ``floor_intra_class_spectral_distance``: two disjoint runs of the real set at the same
        counts; ``classes_used`` (classes behind the intra-class distance), ``left_out`` (fewer than 2 images on either side),
        ``undefined`` (no ring with energy on both sides); ``rejected_real`` / ``rejected_generated`` (labels outside [0, K))."""
        if self.real is None:
            raise RuntimeError("SpectrumEvaluator.evaluate needs prepare_real() first")
        R, K = self.real, self.n_classes
        G = self._set(images, labels)
        if G["shape"] != R["shape"]:
            raise ValueError("spectrum: generated images %s, real images %s" % (G["shape"], R["shape"]))
        out = self._compare(G["pooled"], R["pooled"])
        names = ("spectral_distance",) + DB_NAMES
        per = {name: np.full(K, np.nan) for name in names}
        left = [int(k) for k in range(K) if min(G["count"][k], R["count"][k]) < 2]
        undefined = []
        for k in range(K):
            if k in left:
                continue
            r = self._compare(G["per_class"][k], R["per_class"][k])
            if np.isnan(r["spectral_distance"]):
                undefined.append(k)
                continue
            for name in names:
                per[name][k] = r[name]
        for name in names:
            out["per_class_" + name] = per[name]
            out["intra_class_" + name] = _nanmean(per[name])
        d = per["spectral_distance"][~np.isnan(per["spectral_distance"])]
        out["intra_class_spectral_distance_se"] = float(d.std(ddof=1) / np.sqrt(len(d))) if len(d) >= 2 else float("nan")
        floor_pooled, floor_per = self.floor(G["count"], G["n"])
        out.update(floor_spectral_distance=floor_pooled, floor_per_class_spectral_distance=floor_per,
                   floor_intra_class_spectral_distance=_nanmean(floor_per), classes_used=len(d), left_out=left, undefined=undefined,
                   rejected_real=R["rejected"], rejected_generated=G["rejected"])
        self.last = G
        return out

    def spectra(self):
        """The curves behind the last evaluation: float64 ``real`` / ``generated`` [c,B] and ``real_per_class`` /
        ``generated_per_class`` [K,c,B] (nan rows: empty classes), ``ring_counts`` [B]."""
        if self.real is None or self.last is None:
            raise RuntimeError("SpectrumEvaluator.spectra needs an evaluation first")
        return dict(real=self.real["pooled"], real_per_class=self.real["per_class"], generated=self.last["pooled"],
                    generated_per_class=self.last["per_class"], ring_counts=self.ring_counts.astype(np.int64))

    def close(self):
        self.real = self.last = None
        if self.owns_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = {}
    for key, v in result.items():
        if key in ("left_out", "undefined"):
            out[key] = [int(k) for k in v]
        elif key in ("classes_used", "rejected_real", "rejected_generated"):
            out[key] = int(v)
        elif isinstance(v, np.ndarray):
            out[key] = [nn(e) for e in v]
        else:
            out[key] = nn(v)
    return out


def main(argv=None):
    return standalone(argv, (("real", "the reference set"), ("generated", "the set to score")), (),
                      lambda K, FLAGS, device: SpectrumEvaluator(K, device=device), json_ready)


if __name__ == '__main__':
    main()
