"""Balanced consistency regularisation restated in float64 numpy (the definition is in include/rcgan_hip.h): the reference of
tests/test_bcr_cpu.py (against float64 autograd) and of the GPU tests of rcgan_pair_consistency_fwd_bwd.  Needs no GPU.

One part of pairs rows: x and x_aug [pairs, cols], the scores of an image and of its augmented copy -- cols == 1 where the logit is
already taken at the row's label, the class count with weight rows wts [pairs, cols] (negative entries included).
    c_i = sum_l w[i,l] (x[i,l] - x_aug[i,l])^2,   term = mean_i c_i,   value = lam * term
"""
import numpy as np

ULP = 2.0 ** -23          # fp32 unit in the last place at 1
U32 = 2.0 ** -24          # fp32 unit roundoff


def f64(a):
    return np.asarray(a, np.float64)


def pair_consistency(x, x_aug, wts, lam, scale=1.0):
    """-> dict(value, term, dx, dx_aug, dwts): lam * term, the unweighted mean, and the gradients of the VALUE times `scale` (the
    gradient scale of 16-bit activations: the value itself is never scaled).  dwts is None without weights."""
    x, xa = f64(x), f64(x_aug)
    if x.ndim == 1:
        x, xa = x[:, None], xa[:, None]
    assert x.shape == xa.shape and x.ndim == 2
    pairs = x.shape[0]
    w = np.ones_like(x) if wts is None else f64(wts).reshape(x.shape)
    e = x - xa
    term = float((w * e * e).sum() / pairs)
    dx = scale * lam * 2.0 * w * e / pairs
    return dict(value=lam * term, term=term, dx=dx, dx_aug=-dx, dwts=None if wts is None else scale * lam * e * e / pairs)


def gamma(n):
    """The forward error constant of an fp32 sum of n terms: n u / (1 - n u)."""
    return n * U32 / (1.0 - n * U32)


def bounds(x, x_aug, wts, lam, scale=1.0, dx_before=None, dwts_before=None):
    """Bounds for the fp32 kernel on fp32 inputs, from the number format alone:
       gradients, per element: every factor is a correctly rounded fp32 operation on exact inputs -- the difference e, the coefficient
         2 lam g / pairs (three operations), two products -- so the result is within 6 ulp of its magnitude, 8 taken; where the result
         is added to a buffer (accumulate, dwts) one more rounding of the sum: half an ulp of |before| + |increment|, one taken.
       value: an fp32 sum of pairs * cols terms t = w e^2 / pairs, each formed with four roundings: (gamma_n + 4 ulp) sum |t|, then
         the product by lam: one more ulp of the value."""
    ref = pair_consistency(x, x_aug, wts, lam, scale)
    x2 = f64(x).reshape(ref["dx"].shape)
    w = np.ones_like(x2) if wts is None else f64(wts).reshape(x2.shape)
    e = x2 - f64(x_aug).reshape(x2.shape)
    pairs, n = x2.shape[0], x2.size
    b_dx = 8 * ULP * np.abs(ref["dx"])
    if dx_before is not None:
        b_dx = b_dx + ULP * (np.abs(f64(dx_before).reshape(x2.shape)) + np.abs(ref["dx"]))
    out = dict(dx=b_dx, dx_aug=8 * ULP * np.abs(ref["dx"]))
    if wts is not None:
        before = np.zeros_like(x2) if dwts_before is None else f64(dwts_before).reshape(x2.shape)
        out["dwts"] = 8 * ULP * np.abs(ref["dwts"]) + ULP * (np.abs(before) + np.abs(ref["dwts"]))
    sum_abs = float((np.abs(w) * e * e).sum() / pairs)
    out["term"] = (gamma(n) + 4 * ULP) * sum_abs
    out["value"] = lam * out["term"] + ULP * abs(ref["value"])
    return out
