"""Brute-force float64 restatement of the kernel distance for the tests: the full kernel matrix k(x, y) = (gamma <x, y> + coef0)^3,
its row sums (whole and per segment, with or without the diagonal), the unbiased MMD^2 estimate straight from the definition, the
per-class and subset summaries, and the derived error bound of a row sum computed with an fp32 inner product.  Products of fp32
inputs are exact in float64, so an inner product here carries at most d 2^-53 relative of sum |q_i r_i|.  The product never imports
this module, and this module imports nothing of the product."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma_of(d):
    return 1.0 / d


def dots(q, r):
    return np.asarray(q, np.float64) @ np.asarray(r, np.float64).T


def kernel(q, r, gamma=None, coef0=1.0):
    """[nq, nr] kernel values, float64."""
    g = gamma_of(np.asarray(q).shape[1]) if gamma is None else gamma
    t = g * dots(q, r) + coef0
    return t * t * t


def segments(off, n):
    """Row ranges out of an offset array the way the kernel reads it: clamped to [0, n], a decreasing pair is empty."""
    off = np.clip(np.asarray(off, np.int64), 0, n)
    return [(int(a), int(max(a, b))) for a, b in zip(off[:-1], off[1:])]


def rowsum_segmented(q, q_off, r, r_off, gamma, coef0, exclude_same_row=False):
    """-> (rowsum [nq] float64, written [nq] bool).  exclude_same_row leaves out the pair whose GLOBAL row indices are equal."""
    out, written = np.zeros(len(q)), np.zeros(len(q), bool)
    for (qlo, qhi), (rlo, rhi) in zip(segments(q_off, len(q)), segments(r_off, len(r))):
        written[qlo:qhi] = True
        if qhi == qlo or rhi == rlo:
            continue
        K = kernel(q[qlo:qhi], r[rlo:rhi], gamma, coef0)
        if exclude_same_row:
            K = np.where(np.arange(qlo, qhi)[:, None] == np.arange(rlo, rhi)[None, :], 0.0, K)
        out[qlo:qhi] = K.sum(1)
    return out, written


def row_bound(q, r, gamma, coef0, exclude=None):
    """Per query row: (bound on |computed row sum - exact|, the smallest |k(q_i, r_j)| of the row) for a row sum whose inner
    products are fp32 in any order (|dot_c - dot| <= E = g_d sum_i |q_i r_i|) and everything after them float64:
       sum_j [ 3 (|t| + gamma E)^2 gamma E + 8 2^-53 |t|^3 ] + n 2^-53 sum_j |t|^3.
    exclude [nq, nr] bool: pairs that take no part."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    d = q.shape[1]
    g_d = d * U32 / (1.0 - d * U32)
    E = abs(gamma) * g_d * (np.abs(q) @ np.abs(r).T)                 # gamma E
    t = np.abs(gamma * (q @ r.T) + coef0)
    t3 = t ** 3
    per = 3.0 * (t + E) ** 2 * E + 8.0 * U64 * t3
    smallest = t3.copy()
    if exclude is not None:
        per, t3, smallest = np.where(exclude, 0.0, per), np.where(exclude, 0.0, t3), np.where(exclude, np.inf, smallest)
    n = r.shape[0]
    return per.sum(1) + n * U64 * t3.sum(1), smallest.min(1)


def mmd2_unbiased(g, r, gamma=None, coef0=1.0):
    """The unbiased estimate of MMD^2 between the rows of g and of r; nan with fewer than 2 rows on either side."""
    m, n = len(g), len(r)
    if m < 2 or n < 2:
        return float("nan")
    Kgg, Krr, Kgr = kernel(g, g, gamma, coef0), kernel(r, r, gamma, coef0), kernel(g, r, gamma, coef0)
    s_gg, s_rr = Kgg.sum() - np.trace(Kgg), Krr.sum() - np.trace(Krr)
    return float(s_gg / (m * (m - 1.0)) + s_rr / (n * (n - 1.0)) - 2.0 * Kgr.sum() / (m * float(n)))


def mmd2_biased(g, r, gamma=None, coef0=1.0):
    """The plug-in (V-statistic) estimate: the diagonals stay in and the divisors are m^2 and n^2."""
    return float(kernel(g, g, gamma, coef0).mean() + kernel(r, r, gamma, coef0).mean() - 2.0 * kernel(g, r, gamma, coef0).mean())


def evaluate(real, real_labels, gen, gen_labels, n_classes, subset_size):
    """The evaluator's result by brute force: the full-sample estimate over the rows whose label is in [0, K), per-class values (nan
    where a class has fewer than 2 rows on either side), their mean and standard error, and the estimate on B = min(m, n) //
    subset_size contiguous subsets of the accepted rows in original order."""
    real, gen = np.asarray(real), np.asarray(gen)
    rl, gl = np.asarray(real_labels).reshape(-1), np.asarray(gen_labels).reshape(-1)
    rok, gok = (rl >= 0) & (rl < n_classes), (gl >= 0) & (gl < n_classes)
    R, G = real[rok], gen[gok]
    out = dict(kernel_distance=mmd2_unbiased(G, R))
    per, left = np.full(n_classes, np.nan), []
    for c in range(n_classes):
        r, g = real[rl == c], gen[gl == c]
        if len(r) < 2 or len(g) < 2:
            left.append(c)
            continue
        per[c] = mmd2_unbiased(g, r)
    used = [v for v in per if not np.isnan(v)]
    out["intra_class_kernel_distance"] = float(np.mean(used)) if used else float("nan")
    out["intra_class_kernel_distance_se"] = float(np.std(used, ddof=1) / np.sqrt(len(used))) if len(used) >= 2 else float("nan")
    B = min(len(R), len(G)) // subset_size
    subs = [mmd2_unbiased(G[b * subset_size:(b + 1) * subset_size], R[b * subset_size:(b + 1) * subset_size]) for b in range(B)]
    out.update(subset_mean=float(np.mean(subs)) if B else float("nan"), subset_std=float(np.std(subs)) if B else float("nan"), subsets=B,
               per_class=per, left_out=left, classes_used=n_classes - len(left), rejected_real=int((~rok).sum()),
               rejected_generated=int((~gok).sum()))
    return out
