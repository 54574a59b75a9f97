"""Plain numpy float64 forward and adjoint of the unfused head, loss and softmax entry points of csrc/loss.hip and of
rcgan_bn_infer / rcgan_bn_infer_bwd, written from the formulas of include/rcgan_hip.h (no GPU, no torch).

Every dot-product-like output comes with ``mag``: per element, the sum of the absolute values of the terms that were added, which
the forward error bound of an fp32 sum of L terms in any order needs:  |got - ref| <= (L + 4) * 2^-24 * mag  (``sum_bound``; the
4 covers the roundings around the sum: the products, a division by the count, an offset).  Elementwise results are held to
``elem_bound``: 1e-5 relative per element (the figure of test_head_and_losses, applied per element) plus 1e-37 for results below
the normal fp32 range.

The sigmoid terms are written in their cancellation-free form (``sigmoid_ce_grad``), so the references keep full relative precision
for saturated logits.
"""
import numpy as np

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
HINGE_REAL, HINGE_FAKE, NEG_MEAN, CE_ONES, CE_ZEROS = 0, 1, 2, 3, 4
EPS32 = 2.0 ** -24          # unit roundoff of fp32


def f64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------- tolerances
def sum_bound(L, mag):
    """Forward bound of an fp32 sum of L terms in any order, mag = sum |terms| per element."""
    return (L + 4) * EPS32 * f64(mag)


def elem_bound(ref):
    return 1e-5 * np.abs(f64(ref)) + 1e-37


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (<= 1 passes); inf for a non-finite result."""
    got, ref, bound = f64(got), f64(ref), np.broadcast_to(f64(bound), np.shape(ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------------------------------------------- activations
def act_apply(act, x):
    x = f64(x)
    if act == ACT_RELU:
        return np.where(x > 0, x, 0.0)
    if act == ACT_LRELU:
        return np.maximum(x, 0.2 * x)
    if act == ACT_TANH:
        return np.tanh(x)
    if act == ACT_SIGMOID:
        return sigmoid(x)
    return x.copy()


def act_grad(act, s):
    """The derivative factor: from the sign of s for ReLU / leaky ReLU (s = 0 is the negative side), from the OUTPUT s for tanh / sigmoid."""
    s = f64(s)
    if act == ACT_RELU:
        return np.where(s > 0, 1.0, 0.0)
    if act == ACT_LRELU:
        return np.where(s > 0, 1.0, 0.2)
    if act == ACT_TANH:
        return (1.0 - s) * (1.0 + s)
    if act == ACT_SIGMOID:
        return s * (1.0 - s)
    return np.ones_like(s)


def sigmoid(x):
    """1 / (1 + e^-x) without overflow."""
    x = f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---------------------------------------------------------------------------------------------------- pooled features
def act_meanhw_fwd(x, act):
    """x [n, hw, c] -> feat [n, c] = mean over hw of act(x), mag."""
    a = act_apply(act, x)
    hw = a.shape[1]
    return a.sum(1) / hw, np.abs(a).sum(1) / hw


def act_meanhw_bwd(x, dfeat, act):
    """dx [n, hw, c] = dfeat / hw * act'(x)."""
    x = f64(x)
    return f64(dfeat)[:, None, :] / x.shape[1] * act_grad(act, x)


# ---------------------------------------------------------------------------------------------------- embedding rows
def gather_rows(table, idx):
    return np.asarray(table)[np.asarray(idx)]


def scatter_add_rows(src, idx, v, prev=None):
    """tg [v, d] = (prev or 0) + sum over the rows r with idx[r] == row of src[r]; -> tg, mag."""
    src, idx = f64(src), np.asarray(idx)
    tg = np.zeros((v, src.shape[1])) if prev is None else f64(prev).copy()
    mag = np.abs(tg)
    np.add.at(tg, idx, src)
    np.add.at(mag, idx, np.abs(src))
    return tg, mag


# ---------------------------------------------------------------------------------------------------- projection logits
def proj_logit_fwd(feat, psi, emb):
    """logit[n] = psi[n] + <feat[n], emb[n]> (psi None: no offset); -> logit, mag."""
    pr = f64(feat) * f64(emb)
    off = np.zeros(pr.shape[0]) if psi is None else f64(psi)
    return pr.sum(1) + off, np.abs(pr).sum(1) + np.abs(off)


def proj_logit_bwd(feat, emb, dlogit, dfeat_prev=None):
    """-> dfeat, mag of dfeat (two terms with dfeat_prev), dpsi, demb."""
    g = f64(dlogit)[:, None]
    dfeat = g * f64(emb)
    mag = np.abs(dfeat)
    if dfeat_prev is not None:
        dfeat = dfeat + f64(dfeat_prev)
        mag = mag + np.abs(f64(dfeat_prev))
    return dfeat, mag, f64(dlogit).copy(), g * f64(feat)


def proj_logit_all_fwd(feat, psi, E):
    """logits[n, v] = psi[n] + <feat[n], E[v]>; -> logits, mag."""
    feat, psi, E = f64(feat), f64(psi), f64(E)
    return psi[:, None] + feat @ E.T, np.abs(psi)[:, None] + np.abs(feat) @ np.abs(E).T


def proj_logit_all_bwd(feat, E, dl, dfeat_prev=None):
    """-> (dfeat, mag), (dpsi, mag), (dE, mag): sums over v, v and n."""
    feat, E, dl = f64(feat), f64(E), f64(dl)
    dfeat, mf = dl @ E, np.abs(dl) @ np.abs(E)
    if dfeat_prev is not None:
        dfeat, mf = dfeat + f64(dfeat_prev), mf + np.abs(f64(dfeat_prev))
    return (dfeat, mf), (dl.sum(1), np.abs(dl).sum(1)), (dl.T @ feat, np.abs(dl).T @ np.abs(feat))


# ---------------------------------------------------------------------------------------------------- loss terms
def softplus_neg_abs(x):
    return np.log1p(np.exp(-np.abs(f64(x))))


def sigmoid_ce(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log1p(e^-|x|), z in {0, 1} (arrays allowed)."""
    x = f64(x)
    return np.maximum(x, 0.0) - x * z + softplus_neg_abs(x)


def sigmoid_ce_grad(x, z):
    """d/dx sigmoid_ce = sigmoid(x) - z, as -1 / (1 + e^x) for z = 1 and 1 / (1 + e^-x) for z = 0: neither subtracts numbers near 1."""
    x = f64(x)
    z = np.broadcast_to(f64(z), x.shape)
    return np.where(z != 0, -sigmoid(-x), sigmoid(x))


def loss_term(kind, x):
    """-> term, d term / dx per element."""
    x = f64(x)
    if kind == HINGE_REAL:
        z = 1.0 - x
        return np.where(z > 0, z, 0.0), np.where(z > 0, -1.0, 0.0)
    if kind == HINGE_FAKE:
        z = 1.0 + x
        return np.where(z > 0, z, 0.0), np.where(z > 0, 1.0, 0.0)
    if kind == NEG_MEAN:
        return -x, -np.ones_like(x)
    if kind == CE_ONES:
        return sigmoid_ce(x, 1.0), sigmoid_ce_grad(x, 1.0)
    if kind == CE_ZEROS:
        return sigmoid_ce(x, 0.0), sigmoid_ce_grad(x, 0.0)
    raise ValueError(kind)


def loss_fwd_bwd(kind, x, wts, weight, scale=1.0):
    """x [rows, cols].  Without wts: L = mean over all elements; with wts [rows, cols]: mean over rows of sum over cols of term * wts.
    -> weight * L, its mag, dlogit = scale * weight * dL/dx, dwts = scale * weight * term / rows (what the kernel writes with or
    without wts)."""
    x = f64(x)
    if x.ndim == 1:
        x = x[:, None]
    rows = x.shape[0]
    t, d = loss_term(kind, x)
    wf = f64(wts) / rows if wts is not None else np.full(x.shape, 1.0 / x.size)
    terms = weight * t * wf
    return terms.sum(), np.abs(terms).sum(), scale * weight * d * wf, scale * weight * t / rows


def bce_onehot_fwd_bwd(x, labels, weight, scale=1.0):
    """weight * mean over all elements of sigmoid_ce(x, onehot(labels)); -> value, mag, dx."""
    x = f64(x)
    z = (np.arange(x.shape[1])[None, :] == np.asarray(labels)[:, None]).astype(np.float64)
    terms = weight * sigmoid_ce(x, z) / x.size
    return terms.sum(), np.abs(terms).sum(), scale * weight * sigmoid_ce_grad(x, z) / x.size


# ---------------------------------------------------------------------------------------------------- softmax
def softmax_rows_fwd(l):
    """-> p, the relative bound of p: the exponential and the division elementwise (1e-5), the denominator a sum of cols positive terms."""
    l = f64(l)
    e = np.exp(l - l.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return p, (1e-5 + (l.shape[-1] + 4) * EPS32) * p + 1e-37


def softmax_rows_bwd(p, dp, prev=None):
    """dl = p * (dp - <dp, p>) per row (+ prev).  dp[j] - <dp, p> cancels -- completely at the dominant entry of a saturated row -- so the
    dot product is carried as hi + lo: the products of fp32 inputs are exact in float64, math.fsum adds them exactly (hi, correctly
    rounded) and once more with -hi for what hi lost (lo); dp[j] - hi is exact whenever the two nearly cancel."""
    import math
    p, dp = f64(p), f64(dp)
    assert np.array_equal(p, p.astype(np.float32)) and np.array_equal(dp, dp.astype(np.float32)), "fp32 inputs: exact products"
    pr = (dp * p).reshape(-1, p.shape[-1])
    hi = np.array([math.fsum(r) for r in pr])
    lo = np.array([math.fsum(list(r) + [-h]) for r, h in zip(pr, hi)])
    shape = p.shape[:-1] + (1,)
    dl = p * ((dp - hi.reshape(shape)) - lo.reshape(shape))
    return dl if prev is None else dl + f64(prev)


# ---------------------------------------------------------------------------------------------------- inference batch norm
def bn_infer(x, gamma, beta, mm, mv, eps, act):
    """-> y, the pre-activation value."""
    pre = (f64(x) - f64(mm)) / np.sqrt(f64(mv) + eps) * f64(gamma) + f64(beta)
    return act_apply(act, pre), pre


def bn_infer_bwd(y, dy, gamma, mv, eps, act, prev=None):
    """dx = dy * act'(y) * gamma / sqrt(mv + eps) (+ prev)."""
    g = f64(dy) * (act_grad(act, y) if act != ACT_NONE else 1.0)
    dx = g * f64(gamma) / np.sqrt(f64(mv) + eps)
    return dx if prev is None else dx + f64(prev)


# ---------------------------------------------------------------------------------------------------- fp32 emulations of the two gradient forms
def ce_ones_grad_f32_stable(x):
    """-1 / (1 + expf(x)) in fp32 arithmetic: the stable form written out literally."""
    x = np.asarray(x, np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore"):
        return -one / (one + np.exp(x))


def ce_ones_grad_f32_kernel(x):
    """The same value as csrc/loss.hip evaluates it, from e = expf(-|x|): -e / (1 + e) for x > 0, -1 / (1 + e) otherwise."""
    x = np.asarray(x, np.float32)
    one = np.float32(1.0)
    e = np.exp(-np.abs(x))
    return -np.where(x > 0, e, one) / (one + e)


def ce_ones_grad_f32_subtracted(x):
    """1 / (1 + expf(-x)) - 1 in fp32 arithmetic: the form the kernels used to have."""
    x = np.asarray(x, np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x)) - one
