"""Nearest training images in pixel space: does the generator memorise the training set?

Every other metric of this package (frechet.py, manifold.py, kid.py, msssim.py) scores a generator BETTER the closer its samples lie to
the training set, so replaying training images wins all of them.  The numbers here ask the opposite question.  They rest on one
primitive, ``nearest``: for every query image the nearest reference image under the squared L2 distance of the raw uint8 pixels,
  dist2(a, b) = sum_k (a_k - b_k)^2,
computed EXACTLY by csrc/nn_u8.hip (integer matrix cores; among equally near images the lowest row index wins), pooled or with the
neighbours restricted to the query's class.  With T the clean training set, H a held-out real set, G the generated samples, t(x) the
nearest training image of x and d_X[x] = dist2(x, t(x)):

  rho[t]            squared distance of training image t to its nearest OTHER training image.
  copy_rate         the share of generated images with d_G[g] < rho[t(g)], strictly: g is nearer to a training image than any other
                    training image is (1 - copy_rate is the authenticity of Alaa et al. 2022).  ``copy_rate_heldout`` is the same
                    share of H, the rate fresh real images show; per class with T, H, G and rho restricted to the class.
  nn_distance_z     the data-copying statistic of Meehan et al. 2020: the Mann-Whitney U of d_G against d_H, standardised,
                      U = R_G - n (n + 1) / 2,  var = n m / 12 ((N + 1) - sum_ties (t^3 - t) / (N (N - 1))),  z = (U - n m / 2) / sqrt(var),
                    R_G the sum of the midranks of the n values of d_G among all N = n + m (the distances are integers: ties occur).
                    z far below 0: generated images sit closer to the training set than fresh real images do.
                    ``intra_class_nn_distance_z``: the class values on the class-restricted distances, weighted by the class's share
                    of T, over the classes with at least 20 rows of G and of H; the others are listed in ``left_out``.
  loo_1nn_accuracy  the leave-one-out 1-NN two-sample test (Lopez-Paz & Oquab 2017, Xu et al. 2018) between G and R, the first rows
                    of T class by class, as many per class as G has (and both sides cut to the smaller count): a row is classified
                    correctly if its nearest neighbour in (R u G) minus itself lies on its own side -- its same-side distance strictly
                    smaller; a tie counts 1/2.  0.5: indistinguishable; both sides below 0.5: memorising; generated side near 1:
                    collapsed.  Pooled, and the mean over classes with the neighbours restricted to the class.
  nearest_rmse_median   sqrt(median d_G / d): the typical distance to the nearest training image in pixel units.

Per image set the pixels are uploaded once; one evaluation is 2 + 8 kernel calls (``prepare_real``: 4, once) and the download of 8 bytes per query row.
Everything after the kernel is integer / float64 numpy.

Stand-alone:  python -m rcgan_amd.neighbours --real a.npz --heldout h.npz --generated b.npz [--n_classes K]
(each file: ``images`` [n,32,32,3], [n,3072] CHW rows, [n,28,28,1] or [n,784] of raw pixels 0..255, ``labels`` [n]) prints the numbers
as one JSON line."""
import ctypes as C

import numpy as np

from .evaluators import download, standalone  # noqa: F401  (download: re-exported)
from .msssim import as_uint8_nhwc

MIN_D, MAX_D = 16, 12288                 # the kernel's bounds on the row length, a multiple of 16 (include/rcgan_hip.h)
MIN_CLASS_ROWS = 20                      # rows of a class on either side below which its z is not taken
NO_CANDIDATE = np.uint64(0xFFFFFFFFFFFFFFFF)


def as_rows(images):
    """Images in any layout ``msssim.as_uint8_nhwc`` takes -> uint8 [n, h w c], one fixed pixel order for every set."""
    x = as_uint8_nhwc(images)
    x = x.reshape(len(x), -1)
    if not (MIN_D <= x.shape[1] <= MAX_D) or x.shape[1] % 16:
        raise ValueError("neighbours: rows of %d pixels, expected a multiple of 16 in %d..%d" % (x.shape[1], MIN_D, MAX_D))
    return x


def decode(best):
    """uint64 keys (dist2 << 32 | index, all-ones: no candidate) -> (dist2 int64, index int64), -1 / -1 where no candidate exists."""
    best = np.asarray(best).view(np.uint64).reshape(-1)
    none = best == NO_CANDIDATE
    dist2 = (best >> np.uint64(32)).astype(np.int64)
    index = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dist2[none], index[none] = -1, -1
    return dist2, index


# ------------------------------------------------------------------------------------------------------------- the statistics
def mann_whitney_z(x, y):
    """The standardised Mann-Whitney U of sample x against sample y with midranks and the tie-corrected variance (module docstring);
    nan if a sample is empty or every value is the same."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    n, m = len(x), len(y)
    if n == 0 or m == 0:
        return float("nan")
    N = n + m
    _, inverse, counts = np.unique(np.concatenate([x, y]), return_inverse=True, return_counts=True)
    midrank = np.cumsum(counts) - counts + (counts + 1) / 2.0
    u = midrank[inverse[:n]].sum() - n * (n + 1) / 2.0
    var = n * m / 12.0 * ((N + 1) - float((counts.astype(np.float64) ** 3 - counts).sum()) / (N * (N - 1)))
    if var <= 0:
        return float("nan")
    return float((u - n * m / 2.0) / np.sqrt(var))


def copy_share(dist2, index, rho):
    """The share of the rows whose distance is strictly below rho of their nearest reference row, over the rows where both are
    defined (>= 0); nan if there is none.  -> (share, rows counted)."""
    dist2, index = np.asarray(dist2, np.int64), np.asarray(index, np.int64)
    ok = index >= 0
    ok[ok] = rho[index[ok]] >= 0
    if not ok.any():
        return float("nan"), 0
    return float((dist2[ok] < rho[index[ok]]).mean()), int(ok.sum())


def loo_accuracy(same, other):
    """Leave-one-out 1-NN accuracy of one side: same / other = squared distance to the nearest OTHER row of the own side / to the
    nearest row of the other side, -1 where there is none (counted as infinitely far).  Strictly nearer on the own side: 1, a tie 1/2."""
    same, other = np.asarray(same, np.float64).copy(), np.asarray(other, np.float64).copy()
    if len(same) == 0:
        return float("nan")
    same[same < 0], other[other < 0] = np.inf, np.inf
    return float(((same < other) + 0.5 * (same == other)).mean())


# ------------------------------------------------------------------------------------------------------------- the kernel
class ImageSet:
    """One image set on the device: the rows whose label lies in [0, K) in the caller's order (the pooled segment) and again sorted
    by class (stable, so that inside a class the caller's order holds and the kernel's lowest-index tie rule is the caller's)."""

    def __init__(self, ctx, images, labels, n_classes, is_rows=False):
        """is_rows: ``images`` is already the uint8 [n, d] result of ``as_rows`` (a [n, 3072] array would else be read as CHW rows)."""
        import torch
        x = images if is_rows else as_rows(images)
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        if len(lab) != len(x):
            raise ValueError("neighbours: %d images, %d labels" % (len(x), len(lab)))
        K = int(n_classes)
        self.n_given, self.d, self.n_classes = len(x), x.shape[1], K
        self.kept = np.flatnonzero((lab >= 0) & (lab < K))                  # caller's row of pooled row i
        self.rejected = len(x) - len(self.kept)
        self.labels = lab[self.kept]
        self.order = np.argsort(self.labels, kind="stable")                 # pooled row of class-sorted row i
        self.rows = np.bincount(self.labels, minlength=K).astype(np.int64)
        self.n = len(self.kept)
        self.ctx = ctx
        with torch.cuda.stream(ctx.stream):
            self.pooled = torch.from_numpy(np.ascontiguousarray(x[self.kept])).to(ctx.device)
            self.sorted = self.pooled.index_select(0, torch.from_numpy(self.order).to(ctx.device)) if self.n else self.pooled
            self.off_pooled = torch.tensor([0, self.n], dtype=torch.int32, device=ctx.device)
            self.off_class = torch.from_numpy(np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int32)).to(ctx.device)


def nn_u8(ctx, q, q_off, r, r_off, exclude_same_row):
    """q, r: device uint8 [nq, d], [nr, d]; q_off, r_off: device int32 [n_seg + 1].  -> device int64 [nq] holding the uint64 keys
    dist2 << 32 | reference row (all-ones: no candidate).  Two launches on ``ctx``'s stream, no synchronisation."""
    import torch
    for t, dt in ((q, torch.uint8), (r, torch.uint8), (q_off, torch.int32), (r_off, torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("nn_u8: expected contiguous %s, got %s %s" % (dt, tuple(t.shape), t.dtype))
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1] or q_off.shape != r_off.shape or q_off.dim() != 1:
        raise ValueError("nn_u8: q %s, r %s, offsets %s / %s" % (tuple(q.shape), tuple(r.shape), tuple(q_off.shape), tuple(r_off.shape)))
    with torch.cuda.stream(ctx.stream):
        best = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    ctx.check(ctx.lib.rcgan_nn_u8(ctx.h, q.shape[0], r.shape[0], q.shape[1], q_off.shape[0] - 1, C.c_void_p(q.data_ptr()),
                                  C.c_void_p(q_off.data_ptr()), C.c_void_p(r.data_ptr()), C.c_void_p(r_off.data_ptr()),
                                  1 if exclude_same_row else 0, C.c_void_p(best.data_ptr())))
    return best


def nearest_sets(ctx, qs, rs, per_class=False, exclude_same=False):
    """Nearest row of ImageSet ``rs`` for every row of ImageSet ``qs`` (``exclude_same``: qs is rs and a row's own index is left out).
    -> (dist2 int64 [qs.n_given], index int64 [qs.n_given]): the index counts the rows the CALLER gave for rs; -1 / -1 where no
    neighbour exists -- a dropped row, an empty reference (class), a one-row (class) with exclusion."""
    if qs.d != rs.d or qs.n_classes != rs.n_classes:
        raise ValueError("neighbours: sets of %d and %d pixels, %d and %d classes" % (qs.d, rs.d, qs.n_classes, rs.n_classes))
    if exclude_same and qs is not rs:
        raise ValueError("neighbours: exclude_same needs the same set on both sides")
    dist2, index = np.full(qs.n_given, -1, np.int64), np.full(qs.n_given, -1, np.int64)
    if qs.n == 0 or rs.n == 0:
        return dist2, index
    if per_class:
        best = nn_u8(ctx, qs.sorted, qs.off_class, rs.sorted, rs.off_class, exclude_same)
    else:
        best = nn_u8(ctx, qs.pooled, qs.off_pooled, rs.pooled, rs.off_pooled, exclude_same)
    d2, j = decode(download(ctx, best))
    if per_class:
        j = np.where(j >= 0, rs.order[np.maximum(j, 0)], -1)                # class-sorted row -> pooled row
        back = np.empty_like(d2), np.empty_like(j)
        back[0][qs.order], back[1][qs.order] = d2, j
        d2, j = back
    dist2[qs.kept] = d2
    index[qs.kept] = np.where(j >= 0, rs.kept[np.maximum(j, 0)], -1)        # pooled row -> caller's row
    return dist2, index


def nearest(ctx, q, q_labels, r, r_labels, per_class=False, exclude_same=False, n_classes=None):
    """Host arrays in, host arrays out: uploads both sets (one set when ``exclude_same``: r and r_labels are then ignored), sorts the
    rows by class when ``per_class`` is set, builds the offsets, calls the kernel and decodes.  -> (dist2 int64, index int64 in the
    caller's row order), -1 where undefined."""
    labels = [np.asarray(q_labels).reshape(-1)] + ([] if exclude_same else [np.asarray(r_labels).reshape(-1)])
    K = int(n_classes) if n_classes else int(max(int(l.max()) for l in labels if len(l))) + 1
    qs = ImageSet(ctx, q, q_labels, K)
    rs = qs if exclude_same else ImageSet(ctx, r, r_labels, K)
    return nearest_sets(ctx, qs, rs, per_class, exclude_same)


# ------------------------------------------------------------------------------------------------------------- the evaluator
def class_values(fn, K):
    return np.array([fn(c) for c in range(K)], np.float64)


class NeighbourEvaluator:
    """The memorisation metrics end to end for one run: rho and the held-out distances taken once (``prepare_real``), then
    ``evaluate`` per generated set.  Owns a small runtime Context unless ``ctx`` hands one over."""

    def __init__(self, n_classes, device=0, ctx=None):
        if int(n_classes) < 1:
            raise ValueError("NeighbourEvaluator: n_classes %d (at least 1)" % n_classes)
        self.n_classes = int(n_classes)
        self.owns_ctx = ctx is None
        if ctx is None:
            from .runtime import Context
            ctx = Context(device, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
        self.ctx = ctx
        self.real = None

    def prepare_real(self, train_images, train_labels, heldout_images, heldout_labels):
        """train: the training images with their CLEAN labels; heldout: real images the generator never saw."""
        K = self.n_classes
        T = ImageSet(self.ctx, train_images, train_labels, K)
        H = ImageSet(self.ctx, heldout_images, heldout_labels, K)
        if T.d != H.d:
            raise ValueError("neighbours: training rows of %d pixels, held-out rows of %d" % (T.d, H.d))
        real = dict(T=T, H=H, images=as_rows(train_images), labels=np.asarray(train_labels).reshape(-1).astype(np.int64),
                    H_labels=np.asarray(heldout_labels).reshape(-1).astype(np.int64))
        real["rho"], _ = nearest_sets(self.ctx, T, T, False, True)
        real["rho_class"], _ = nearest_sets(self.ctx, T, T, True, True)
        real["d_H"], real["t_H"] = nearest_sets(self.ctx, H, T, False, False)
        real["d_H_class"], real["t_H_class"] = nearest_sets(self.ctx, H, T, True, False)
        real["copy_rate_heldout"], _ = copy_share(real["d_H"], real["t_H"], real["rho"])
        real["copy_rate_heldout_per_class"] = class_values(
            lambda c: copy_share(real["d_H_class"][real["H_labels"] == c], real["t_H_class"][real["H_labels"] == c], real["rho_class"])[0], K)
        self.real = real
        return real

    def loo(self, G, g_images, g_labels):
        """The leave-one-out 1-NN accuracies between G and the first rows of T, class by class (module docstring)."""
        K, real = self.n_classes, self.real
        T = real["T"]
        take = np.minimum(G.rows, T.rows)
        first = lambda lab: np.sort(np.concatenate([np.flatnonzero(lab == c)[:take[c]] for c in range(K)]).astype(np.int64))
        g_lab = np.asarray(g_labels).reshape(-1).astype(np.int64)
        gi, ri = first(g_lab), first(real["labels"])
        out = dict(loo_rows=int(len(gi)))
        if len(gi) == 0:
            nan = float("nan")
            out.update(loo_1nn_accuracy=nan, loo_1nn_accuracy_real=nan, loo_1nn_accuracy_generated=nan, intra_class_loo_1nn_accuracy=nan,
                       loo_1nn_accuracy_per_class=np.full((K, 2), np.nan))
            return out
        Gs = G if len(gi) == G.n_given else ImageSet(self.ctx, as_rows(g_images)[gi], g_lab[gi], K, is_rows=True)
        Rs = ImageSet(self.ctx, real["images"][ri], real["labels"][ri], K, is_rows=True)
        lab_g, lab_r = g_lab[gi], real["labels"][ri]
        acc = {}
        for per_class in (False, True):
            gg, _ = nearest_sets(self.ctx, Gs, Gs, per_class, True)
            rr, _ = nearest_sets(self.ctx, Rs, Rs, per_class, True)
            gr, _ = nearest_sets(self.ctx, Gs, Rs, per_class, False)
            rg, _ = nearest_sets(self.ctx, Rs, Gs, per_class, False)
            acc[per_class] = (rr, rg, gg, gr)
        rr, rg, gg, gr = acc[False]
        a_r, a_g = loo_accuracy(rr, rg), loo_accuracy(gg, gr)
        rr, rg, gg, gr = acc[True]
        per = np.array([[loo_accuracy(rr[lab_r == c], rg[lab_r == c]), loo_accuracy(gg[lab_g == c], gr[lab_g == c])] if take[c] >= 2
                        else [np.nan, np.nan] for c in range(K)], np.float64).reshape(K, 2)
        used = per[~np.isnan(per[:, 0])]
        out.update(loo_1nn_accuracy=0.5 * (a_r + a_g), loo_1nn_accuracy_real=a_r, loo_1nn_accuracy_generated=a_g,
                   intra_class_loo_1nn_accuracy=float(used.mean()) if len(used) else float("nan"), loo_1nn_accuracy_per_class=per)
        return out

    def evaluate(self, images, labels):
        """-> dict: ``copy_rate`` / ``copy_rate_heldout`` (pooled), ``copy_rate_per_class`` / ``copy_rate_heldout_per_class`` [K] (nan
        where a side has no row), ``classes_above_heldout`` of ``classes_compared``; ``nn_distance_z`` (pooled),
        ``nn_distance_z_per_class`` [K] (nan where left out), ``intra_class_nn_distance_z`` (nan if every class is left out),
        ``classes_used``, ``left_out``; ``loo_1nn_accuracy`` with ``_real`` and ``_generated``, ``intra_class_loo_1nn_accuracy`` and
        ``loo_1nn_accuracy_per_class`` [K, 2] (real, generated); ``nearest_rmse_median`` / ``nearest_rmse_median_heldout``;
        ``nearest_index`` / ``nearest_dist2`` [n] (the pooled nearest training row of every generated row, -1 for a dropped row);
        ``rejected_real`` / ``rejected_heldout`` / ``rejected_generated`` (rows whose label was outside [0, K), dropped)."""
        if self.real is None:
            raise RuntimeError("NeighbourEvaluator.evaluate needs prepare_real() first")
        K, real = self.n_classes, self.real
        T, H = real["T"], real["H"]
        G = ImageSet(self.ctx, images, labels, K)
        if G.d != T.d:
            raise ValueError("neighbours: generated rows of %d pixels, training rows of %d" % (G.d, T.d))
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        d_G, t_G = nearest_sets(self.ctx, G, T, False, False)
        d_Gc, t_Gc = nearest_sets(self.ctx, G, T, True, False)
        out = dict(nearest_index=t_G, nearest_dist2=d_G)
        out["copy_rate"], _ = copy_share(d_G, t_G, real["rho"])
        out["copy_rate_heldout"] = real["copy_rate_heldout"]
        per = class_values(lambda c: copy_share(d_Gc[lab == c], t_Gc[lab == c], real["rho_class"])[0], K)
        held = real["copy_rate_heldout_per_class"]
        both = ~np.isnan(per) & ~np.isnan(held)
        out.update(copy_rate_per_class=per, copy_rate_heldout_per_class=held, classes_above_heldout=int((per[both] > held[both]).sum()),
                   classes_compared=int(both.sum()))
        ok_g, ok_h = d_G >= 0, real["d_H"] >= 0
        out["nn_distance_z"] = mann_whitney_z(d_G[ok_g], real["d_H"][ok_h])
        okc_g, okc_h = d_Gc >= 0, real["d_H_class"] >= 0
        z = np.full(K, np.nan)
        for c in range(K):
            a, b = d_Gc[okc_g & (lab == c)], real["d_H_class"][okc_h & (real["H_labels"] == c)]
            if len(a) >= MIN_CLASS_ROWS and len(b) >= MIN_CLASS_ROWS:
                z[c] = mann_whitney_z(a, b)
        used = ~np.isnan(z)
        share = T.rows / max(T.n, 1)
        out.update(nn_distance_z_per_class=z, classes_used=int(used.sum()), left_out=[int(c) for c in range(K) if not used[c]],
                   intra_class_nn_distance_z=float((z[used] * share[used]).sum() / share[used].sum()) if used.any() and share[used].sum() > 0
                   else float("nan"))
        out.update(self.loo(G, images, labels))
        rmse = lambda v: float(np.sqrt(np.median(v) / T.d)) if len(v) else float("nan")
        out.update(nearest_rmse_median=rmse(d_G[ok_g]), nearest_rmse_median_heldout=rmse(real["d_H"][ok_h]),
                   rejected_real=T.rejected, rejected_heldout=H.rejected, rejected_generated=G.rejected)
        return out

    def nearest_training_rows(self, images):
        """The pooled nearest training row of every image, whatever its class -> (dist2, index into the training rows given)."""
        T = self.real["T"]
        Q = ImageSet(self.ctx, images, np.zeros(len(images), np.int64), self.n_classes)
        return nearest_sets(self.ctx, Q, T, False, False)

    def close(self):
        self.real = None
        if self.owns_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None


SCALARS = ("copy_rate", "copy_rate_heldout", "nn_distance_z", "intra_class_nn_distance_z", "loo_1nn_accuracy", "loo_1nn_accuracy_real",
           "loo_1nn_accuracy_generated", "intra_class_loo_1nn_accuracy", "nearest_rmse_median", "nearest_rmse_median_heldout")


def json_ready(result):
    nn = lambda v: None if np.isnan(v) else float(v)
    out = dict(result)
    for key in SCALARS:
        out[key] = nn(result[key])
    for key in ("copy_rate_per_class", "copy_rate_heldout_per_class", "nn_distance_z_per_class"):
        out[key] = [nn(v) for v in result[key]]
    out["loo_1nn_accuracy_per_class"] = [[nn(v) for v in row] for row in result["loo_1nn_accuracy_per_class"]]
    for key in ("nearest_index", "nearest_dist2", "left_out"):
        out[key] = [int(v) for v in result[key]]
    for key in ("classes_above_heldout", "classes_compared", "classes_used", "loo_rows", "rejected_real", "rejected_heldout", "rejected_generated"):
        out[key] = int(result[key])
    return out


def main(argv=None):
    return standalone(argv, (("real", "the training set"), ("heldout", "real images the generator never saw"), ("generated", "the set to score")),
                      (), lambda K, FLAGS, device: NeighbourEvaluator(K, device=device), json_ready)


if __name__ == '__main__':
    main()
