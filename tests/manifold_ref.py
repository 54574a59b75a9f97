"""Brute-force float64 restatement of the k-NN manifold metrics for the tests: the full distance matrix, radii as the (k+1)-th smallest
entry of a row of the set's self-distance matrix (self included), ball counts, nearest distances, and precision / recall / density /
coverage pooled and per class.  Differences are formed in float64 from the fp32 inputs, so a distance here is exact to 2^-53 relative
per term.  The product never imports this module, and this module imports nothing of the product."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

METRICS = ("precision", "recall", "density", "coverage")
THREADS = max(1, min(16, os.cpu_count() or 1))


def dist2(a, b):
    """[na, nb] squared distances, float64, as the direct sum of squared differences."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((len(a), len(b)))
    step = max(1, (1 << 21) // max(1, len(b) * a.shape[1]))          # rows of a at a time: a difference tensor stays ~16 MB

    def block(lo):
        diff = a[lo:lo + step, None, :] - b[None, :, :]
        out[lo:lo + step] = np.einsum("ijk,ijk->ij", diff, diff)
    starts = range(0, len(a), step)
    if len(a) * len(b) * a.shape[1] < (1 << 24):
        for lo in starts:
            block(lo)
    else:                                                            # (numpy releases the interpreter lock inside both operations)
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            list(pool.map(block, starts))
    return out


def radii(x, k):
    """Squared distance from every row to its k-th nearest OTHER row, duplicates counted; -1 for every row when the set has <= k rows."""
    n = len(x)
    if n <= k:
        return np.full(n, -1.0)
    return np.partition(dist2(x, x), k, axis=1)[:, k]          # (entry k of the sorted row, without sorting the rest)


def counts_nearest(q, r, r_radius2):
    """For every row of q: (#{ j : dist2(q_i, r_j) <= r_radius2[j] }, min_j dist2(q_i, r_j)); an empty r gives (0, +inf)."""
    if len(r) == 0:
        return np.zeros(len(q), np.int64), np.full(len(q), np.inf)
    D = dist2(q, r)
    rad = np.asarray(r_radius2, np.float64)
    return ((D <= rad[None, :]) & (rad[None, :] >= 0)).sum(1), D.min(1)


def segments(off, n):
    """Row ranges out of an offset array the way the kernel reads it: clamped to [0, n], a decreasing pair is empty."""
    off = np.clip(np.asarray(off, np.int64), 0, n)
    return [(int(a), int(max(a, b))) for a, b in zip(off[:-1], off[1:])]


def radii_segmented(x, off, k):
    """-> (radius2 [n] float64, written [n] bool: rows some segment covers)."""
    out, written = np.zeros(len(x)), np.zeros(len(x), bool)
    for lo, hi in segments(off, len(x)):
        out[lo:hi], written[lo:hi] = radii(x[lo:hi], k), True
    return out, written


def ball_segmented(q, q_off, r, r_off, r_radius2):
    """-> (count [nq] int64, nearest2 [nq] float64, written [nq] bool)."""
    cnt, near, written = np.zeros(len(q), np.int64), np.zeros(len(q)), np.zeros(len(q), bool)
    for (qlo, qhi), (rlo, rhi) in zip(segments(q_off, len(q)), segments(r_off, len(r))):
        cnt[qlo:qhi], near[qlo:qhi] = counts_nearest(q[qlo:qhi], r[rlo:rhi], np.asarray(r_radius2)[rlo:rhi])
        written[qlo:qhi] = True
    return cnt, near, written


def undecided(q, q_off, r, r_off, r_radius2, eps):
    """Per query row: (pairs decided inside, undecided pairs) where a pair is undecided when its float64 distance lies within eps
    relative of the radius it is compared with (a negative radius is decided: never inside)."""
    inside, open_ = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    rad_all = np.asarray(r_radius2, np.float64)
    for (qlo, qhi), (rlo, rhi) in zip(segments(q_off, len(q)), segments(r_off, len(r))):
        if qhi == qlo or rhi == rlo:
            continue
        D, rad = dist2(q[qlo:qhi], r[rlo:rhi]), rad_all[rlo:rhi][None, :]
        und = (np.abs(D - rad) <= eps * rad) & (rad >= 0)
        inside[qlo:qhi] = ((D <= rad) & (rad >= 0) & ~und).sum(1)
        open_[qlo:qhi] = und.sum(1)
    return inside, open_


def metrics_of(real, gen, k):
    """precision / recall / density / coverage of two feature sets, straight from the definitions; nan when either has <= k rows."""
    if len(real) <= k or len(gen) <= k:
        return {m: float("nan") for m in METRICS}
    D = dist2(gen, real)                                  # [n_g, n_r]
    rad_r, rad_g = radii(real, k), radii(gen, k)
    in_real = D <= rad_r[None, :]                         # g inside the ball of r
    in_gen = D <= rad_g[:, None]                          # r inside the ball of g
    return dict(precision=float(in_real.any(1).mean()), recall=float(in_gen.any(0).mean()),
                density=float(in_real.sum() / (k * len(gen))), coverage=float((D.min(0) <= rad_r).mean()))


def evaluate(real, real_labels, gen, gen_labels, n_classes, k):
    """The evaluator's result by brute force: pooled metrics over the rows whose label is in [0, K), per-class arrays (nan where a
    class has <= k rows on either side), their means, the classes left out and the rejected rows."""
    real, gen = np.asarray(real), np.asarray(gen)
    rl, gl = np.asarray(real_labels).reshape(-1), np.asarray(gen_labels).reshape(-1)
    rok, gok = (rl >= 0) & (rl < n_classes), (gl >= 0) & (gl < n_classes)
    out = metrics_of(real[rok], gen[gok], k)
    per = {m: np.full(n_classes, np.nan) for m in METRICS}
    left = []
    for c in range(n_classes):
        r, g = real[rl == c], gen[gl == c]
        if len(r) <= k or len(g) <= k:
            left.append(c)
            continue
        for m, v in metrics_of(r, g, k).items():
            per[m][c] = v
    for m in METRICS:
        out["intra_class_" + m] = float(np.mean([v for v in per[m] if not np.isnan(v)])) if len(left) < n_classes else float("nan")
    out.update(per_class=per, left_out=left, classes_used=n_classes - len(left), rejected_real=int((~rok).sum()),
               rejected_generated=int((~gok).sum()))
    return out
