"""Float64 restatement of the diversity-sensitive generator term on same-label pairs (include/rcgan_hip.h,
rcgan_pair_diversity_fwd_bwd): the reference of the GPU tests, itself checked against float64 autograd in tests/test_diversity_cpu.py.

For x [2P, D], z [2P, Z], pair i = rows (i, i + P):
    dI_i = mean_k |x[i,k] - x[i+P,k]|,  dz_i = mean_k |z[i,k] - z[i+P,k]|,  r_i = dI_i / dz_i
    m_i  = 0 if labels are given and differ, or dz_i == 0; else 1
    loss = -(weight / P) sum_i m_i min(r_i, tau)
    dx[i,k] = -c_i sgn(x[i,k] - x[i+P,k]),  dx[i+P,k] = +c_i sgn(...),  c_i = m_i [r_i < tau] weight scale / (P D dz_i)
"""
import numpy as np


def pair_diversity(x, z, labels, weight, tau, scale=1.0):
    """-> dict(loss, ratio [P] (-1 where masked), raw [P] (the ratio of every pair with dz > 0, nan otherwise), mask [P] bool (True =
    the pair counts), clamped [P] bool, terms [P] (m_i min(r_i, tau)), c [P], dx [2P, D]); everything float64.  scale multiplies the
    gradient only."""
    x = np.asarray(x, np.float64)
    z = np.asarray(z, np.float64)
    n, d = x.shape
    assert n % 2 == 0 and z.shape[0] == n
    p = n // 2
    diff = x[:p] - x[p:]
    di = np.abs(diff).mean(1)
    dz = np.abs(z[:p] - z[p:]).mean(1)
    mask = dz != 0
    if labels is not None:
        labels = np.asarray(labels)
        mask &= labels[:p] == labels[p:]
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.where(dz != 0, di / np.where(dz != 0, dz, 1.0), np.nan)
    r = np.where(mask, raw, 0.0)
    clamped = mask & (r >= tau)
    terms = np.where(mask, np.minimum(r, tau), 0.0)
    loss = -(weight / p) * terms.sum()
    push = mask & ~clamped
    c = np.where(push, weight * scale / (p * d * np.where(dz != 0, dz, 1.0)), 0.0)
    g = -c[:, None] * np.sign(diff)
    return dict(loss=float(loss), ratio=np.where(mask, r, -1.0), raw=raw, mask=mask, clamped=clamped, terms=terms, c=c,
                dx=np.concatenate([g, -g], 0))


def report(ratio, tau):
    """CifarRCGAN.diversity_report() from a ratio buffer: the mean over unmasked pairs, the shares of B clamped and masked."""
    ratio = np.asarray(ratio, np.float64)
    live = ratio >= 0
    return dict(ratio_mean=float(ratio[live].mean()) if live.any() else None,
                clamped=float(np.count_nonzero(live & (ratio >= tau))) / ratio.size, masked=float(np.count_nonzero(~live)) / ratio.size)


def min_relative_gap_to_tau(res, tau):
    """The smallest |r_i - tau| / tau over the unmasked pairs (inf for tau = inf or no such pair): the tests assert it is >= 1e-3, so
    that no pair's side of the clamp depends on rounding."""
    if not np.isfinite(tau) or not res["mask"].any():
        return np.inf
    return float(np.min(np.abs(res["raw"][res["mask"]] - tau)) / tau)
