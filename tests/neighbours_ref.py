"""Brute-force restatement of rcgan_nn_u8 (csrc/nn_u8.hip) and of the statistics of rcgan_amd/neighbours.py, numpy only.

Distances: the Gram matrix of the raw pixel values in float64 -- every entry an integer below 12288 * 255^2 < 2^30, far below 2^53, so
the float64 products and sums are exact -- then |a|^2 + |b|^2 - 2 a.b as int64.  The key is dist2 * 2^32 + j in int64 (below 2^62);
an excluded or non-existent candidate gets the distance SENTINEL = 2^31 - 1 (above every real distance, and small enough for the
shift), and a row whose minimum is still the sentinel has no candidate: all-ones, as the kernel writes it.

Everything is written independently of neighbours.py: ranks by sorting and walking the tie groups, accuracies by explicit comparison."""
import numpy as np

SENTINEL = 2 ** 31 - 1
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MIN_CLASS_ROWS = 20


def pair_dist2(a, b):
    """uint8 [n, d], [m, d] -> int64 [n, m] of exact squared distances."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (a @ b.T)
    out = np.rint(d).astype(np.int64)
    assert (out == d).all() and (out >= 0).all()
    return out


def clamp_segments(off, n):
    """The kernel's reading of an offset array: every entry clamped to [0, n], a decreasing pair an empty segment."""
    off = np.clip(np.asarray(off, np.int64), 0, n)
    return [(int(a), int(max(a, b))) for a, b in zip(off[:-1], off[1:])]


def best(q, r, q_off=None, r_off=None, exclude=False, fill=ALL_ONES):
    """-> uint64 [nq]: what rcgan_nn_u8 leaves in a ``best`` array that held ``fill`` everywhere before the call."""
    q, r = np.asarray(q, np.uint8), np.asarray(r, np.uint8)
    out = np.full(len(q), fill, np.uint64)
    q_off = [0, len(q)] if q_off is None else q_off
    r_off = [0, len(r)] if r_off is None else r_off
    for (qs, qe), (rs, re) in zip(clamp_segments(q_off, len(q)), clamp_segments(r_off, len(r))):
        if qe <= qs:
            continue
        out[qs:qe] = ALL_ONES
        if re <= rs:
            continue
        d = pair_dist2(q[qs:qe], r[rs:re])
        j = np.arange(rs, re, dtype=np.int64)
        if exclude:
            d[np.arange(qs, qe)[:, None] == j[None, :]] = SENTINEL
        key = (d * 2 ** 32 + j[None, :]).min(axis=1)
        have = (key >> 32) != SENTINEL
        out[qs:qe][have] = key[have].astype(np.uint64)
    return out


def best_triple_loop(q, r, q_off, r_off, exclude, fill=ALL_ONES):
    """The same by three nested loops of Python integers (tiny inputs only)."""
    out = [int(fill)] * len(q)
    for (qs, qe), (rs, re) in zip(clamp_segments(q_off, len(q)), clamp_segments(r_off, len(r))):
        for i in range(qs, qe):
            key = int(ALL_ONES)
            for j in range(rs, re):
                if exclude and i == j:
                    continue
                d = 0
                for k in range(len(q[i])):
                    d += (int(q[i][k]) - int(r[j][k])) ** 2
                key = min(key, (d << 32) | j)
            out[i] = key
    return np.array(out, np.uint64)


def nearest(q, ql, r, rl, K, per_class, exclude):
    """Rows in the caller's order with labels; -> (dist2, index) int64, -1 where no neighbour exists (a label outside [0, K) drops a
    row from either side).  Lowest index among equally near rows."""
    q, r, ql, rl = np.asarray(q, np.uint8), np.asarray(r, np.uint8), np.asarray(ql, np.int64), np.asarray(rl, np.int64)
    dist2, index = np.full(len(q), -1, np.int64), np.full(len(q), -1, np.int64)
    okq, okr = (ql >= 0) & (ql < K), (rl >= 0) & (rl < K)
    groups = [(np.flatnonzero(ql == c), np.flatnonzero(rl == c)) for c in range(K)] if per_class else [(np.flatnonzero(okq), np.flatnonzero(okr))]
    for qi, ri in groups:
        if len(qi) == 0 or len(ri) == 0:
            continue
        d = pair_dist2(q[qi], r[ri])
        if exclude:
            d[qi[:, None] == ri[None, :]] = SENTINEL
        key = (d * 2 ** 32 + ri[None, :]).min(axis=1)
        have = (key >> 32) != SENTINEL
        dist2[qi[have]], index[qi[have]] = key[have] >> 32, key[have] & 0xFFFFFFFF
    return dist2, index


def mann_whitney_z(x, y):
    """Standardised U of x against y: midranks by walking the tie groups of the sorted pooled sample."""
    x, y = [float(v) for v in x], [float(v) for v in y]
    n, m = len(x), len(y)
    if n == 0 or m == 0:
        return float("nan")
    pooled = sorted([(v, 0) for v in x] + [(v, 1) for v in y])
    N = n + m
    rank_sum, ties, a = 0.0, 0.0, 0
    while a < N:
        b = a
        while b < N and pooled[b][0] == pooled[a][0]:
            b += 1
        t = b - a
        mid = (a + 1 + b) / 2.0                                    # ranks a + 1 .. b
        rank_sum += mid * sum(1 for k in range(a, b) if pooled[k][1] == 0)
        ties += t ** 3 - t
        a = b
    u = rank_sum - n * (n + 1) / 2.0
    var = n * m / 12.0 * ((N + 1) - ties / (N * (N - 1.0)))
    return (u - n * m / 2.0) / np.sqrt(var) if var > 0 else float("nan")


def _copy_rate(d, t, rho):
    ok = [k for k in range(len(d)) if t[k] >= 0 and rho[t[k]] >= 0]
    return float(np.mean([d[k] < rho[t[k]] for k in ok])) if ok else float("nan")


def _loo(same, other):
    if len(same) == 0:
        return float("nan")
    inf = lambda v: np.inf if v < 0 else float(v)
    return float(np.mean([1.0 if inf(s) < inf(o) else (0.5 if inf(s) == inf(o) else 0.0) for s, o in zip(same, other)]))


def prepare(T, lt, H, lh, K):
    """What does not depend on the generated set: rho and the held-out distances, pooled and per class (computed once per module)."""
    T, H = np.asarray(T, np.uint8), np.asarray(H, np.uint8)
    lt, lh = np.asarray(lt, np.int64).reshape(-1), np.asarray(lh, np.int64).reshape(-1)
    return dict(rho=nearest(T, lt, T, lt, K, False, True)[0], rho_c=nearest(T, lt, T, lt, K, True, True)[0],
                h=nearest(H, lh, T, lt, K, False, False), hc=nearest(H, lh, T, lt, K, True, False))


def evaluate(T, lt, H, lh, G, lg, K, real=None):
    """The numbers of NeighbourEvaluator.prepare_real(T, lt, H, lh) + evaluate(G, lg) by brute force; images as uint8 rows [n, d] in
    one pixel order.  real: the result of ``prepare`` on the same T and H, to share it among several generated sets."""
    real = prepare(T, lt, H, lh, K) if real is None else real
    T, H, G = (np.asarray(v, np.uint8) for v in (T, H, G))
    lt, lh, lg = (np.asarray(v, np.int64).reshape(-1) for v in (lt, lh, lg))
    rho, rho_c, (d_h, t_h), (d_hc, t_hc) = real["rho"], real["rho_c"], real["h"], real["hc"]
    d_g, t_g = nearest(G, lg, T, lt, K, False, False)
    d_gc, t_gc = nearest(G, lg, T, lt, K, True, False)
    out = dict(nearest_index=t_g, nearest_dist2=d_g, copy_rate=_copy_rate(d_g, t_g, rho), copy_rate_heldout=_copy_rate(d_h, t_h, rho))
    per = np.array([_copy_rate(d_gc[lg == c], t_gc[lg == c], rho_c) for c in range(K)])
    held = np.array([_copy_rate(d_hc[lh == c], t_hc[lh == c], rho_c) for c in range(K)])
    both = ~np.isnan(per) & ~np.isnan(held)
    out.update(copy_rate_per_class=per, copy_rate_heldout_per_class=held, classes_above_heldout=int((per[both] > held[both]).sum()),
               classes_compared=int(both.sum()))
    out["nn_distance_z"] = mann_whitney_z(d_g[d_g >= 0], d_h[d_h >= 0])
    z, weight = np.full(K, np.nan), np.zeros(K)
    for c in range(K):
        a, b = d_gc[(lg == c) & (d_gc >= 0)], d_hc[(lh == c) & (d_hc >= 0)]
        if len(a) >= MIN_CLASS_ROWS and len(b) >= MIN_CLASS_ROWS:
            z[c], weight[c] = mann_whitney_z(a, b), (lt == c).sum()
    used = ~np.isnan(z)
    out.update(nn_distance_z_per_class=z, classes_used=int(used.sum()), left_out=[c for c in range(K) if not used[c]],
               intra_class_nn_distance_z=float((z[used] * weight[used]).sum() / weight[used].sum()) if used.any() else float("nan"))
    # leave-one-out 1-NN: the first rows of T per class, as many as G has of the class; both sides cut to the smaller count
    gi, ri = [], []
    for c in range(K):
        n_c = min(int((lg == c).sum()), int((lt == c).sum()))
        gi += np.flatnonzero(lg == c)[:n_c].tolist()
        ri += np.flatnonzero(lt == c)[:n_c].tolist()
    gi, ri = np.array(sorted(gi), np.int64), np.array(sorted(ri), np.int64)
    Gs, gl, Rs, rl = G[gi], lg[gi], T[ri], lt[ri]
    acc = {}
    for per_class in (False, True):
        acc[per_class] = (nearest(Rs, rl, Rs, rl, K, per_class, True)[0], nearest(Rs, rl, Gs, gl, K, per_class, False)[0],
                          nearest(Gs, gl, Gs, gl, K, per_class, True)[0], nearest(Gs, gl, Rs, rl, K, per_class, False)[0])
    rr, rg, gg, gr = acc[False]
    out.update(loo_rows=len(gi), loo_1nn_accuracy_real=_loo(rr, rg), loo_1nn_accuracy_generated=_loo(gg, gr))
    out["loo_1nn_accuracy"] = 0.5 * (out["loo_1nn_accuracy_real"] + out["loo_1nn_accuracy_generated"])
    rr, rg, gg, gr = acc[True]
    per = np.array([[_loo(rr[rl == c], rg[rl == c]), _loo(gg[gl == c], gr[gl == c])] if (gl == c).sum() >= 2 else [np.nan, np.nan]
                    for c in range(K)]).reshape(K, 2)
    out["loo_1nn_accuracy_per_class"] = per
    ok = ~np.isnan(per[:, 0])
    out["intra_class_loo_1nn_accuracy"] = float(per[ok].mean()) if ok.any() else float("nan")
    d = T.shape[1]
    out.update(nearest_rmse_median=float(np.sqrt(np.median(d_g[d_g >= 0]) / d)), nearest_rmse_median_heldout=float(np.sqrt(np.median(d_h[d_h >= 0]) / d)),
               rejected_real=int(((lt < 0) | (lt >= K)).sum()), rejected_heldout=int(((lh < 0) | (lh >= K)).sum()),
               rejected_generated=int(((lg < 0) | (lg >= K)).sum()))
    return out
