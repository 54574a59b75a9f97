"""Float64 numpy restatement of multi-scale SSIM as the reference's cifar10/common/msssim.py computes it (max_val 255, k1 0.01,
k2 0.03, five scales, an 11-tap Gaussian window shrunk to the level's size), with direct sliding windows: no FFT, no scipy.

``pair_scales`` gives what ``_SSIMForMultiScale`` returns for a batch of ONE pair at each of the five levels ``MultiScaleSSIM`` walks
(as [2, 5]: row 0 the contrast-structure means, row 1 the SSIM means); ``combine`` is ``MultiScaleSSIM`` of a batch of pairs out of
those per-pair values: all pairs of a batch have equally many positions, so the batch's mean per scale is the mean of the pairs' means."""
import numpy as np

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
LEVELS = 5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def taps(size):
    """The 1-D factor of the reference's 'fspecial' window of ``size`` taps and sigma 1.5 size / 11: the 2-D window is its outer
    product with itself (exp(-(x^2 + y^2) / 2 sigma^2) over its sum; half-integer centres for an even size)."""
    sigma = 1.5 * size / 11.0
    x = np.arange(size, dtype=np.float64) - 0.5 * (size - 1)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def _filter(x, g):
    """'valid' separable filtering of [h, w, c] with the taps g along h and w."""
    s = len(g)
    h, w = x.shape[:2]
    rows = sum(g[k] * x[:, k:k + w - s + 1] for k in range(s))
    return sum(g[k] * rows[k:k + h - s + 1] for k in range(s))


def _half(x):
    """2 x 2 mean at stride 2 anchored at (0, 0); an odd size repeats its last row / column."""
    if x.shape[0] % 2:
        x = np.concatenate([x, x[-1:]], axis=0)
    if x.shape[1] % 2:
        x = np.concatenate([x, x[:, -1:]], axis=1)
    return 0.25 * (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])


def ssim_cs(a, b):
    """(ssim, cs) of one pair [h, w, c] at ONE scale."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = taps(min(11, a.shape[0], a.shape[1]))
    mu1, mu2 = _filter(a, g), _filter(b, g)
    s11, s22, s12 = _filter(a * a, g) - mu1 * mu1, _filter(b * b, g) - mu2 * mu2, _filter(a * b, g) - mu1 * mu2
    v1, v2 = 2.0 * s12 + C2, s11 + s22 + C2
    return float(np.mean((2.0 * mu1 * mu2 + C1) * v1 / ((mu1 * mu1 + mu2 * mu2 + C1) * v2))), float(np.mean(v1 / v2))


def pair_scales(a, b):
    """[2, 5] of one pair [h, w, c]: row 0 cs, row 1 ssim, per level."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((2, LEVELS))
    for l in range(LEVELS):
        out[1, l], out[0, l] = ssim_cs(a, b)
        a, b = _half(a), _half(b)
    return out


def scales(images, pairs):
    """[P, 2, 5] for images [n, h, w, c] and index pairs [P, 2]; a pair with an index outside [0, n) is nan."""
    images, pairs = np.asarray(images), np.asarray(pairs).reshape(-1, 2)
    out = np.full((len(pairs), 2, LEVELS), np.nan)
    for p, (i, j) in enumerate(pairs):
        if 0 <= i < len(images) and 0 <= j < len(images):
            out[p] = pair_scales(images[i], images[j])
    return out


def combine(sc):
    """MultiScaleSSIM of the batch whose per-pair values are sc [P, 2, 5]; nan where a power's base is not positive (the reference
    raises a negative number to a fractional power there: nan too)."""
    sc = np.asarray(sc, np.float64).reshape(-1, 2, LEVELS)
    if len(sc) == 0:
        return float("nan")
    m = sc.mean(axis=0)
    base = np.concatenate([m[0, :LEVELS - 1], m[1, LEVELS - 1:]])
    if not (base > 0).all():
        return float("nan")
    return float(np.prod(base ** WEIGHTS))


def msssim(img1, img2):
    """MultiScaleSSIM(img1, img2) of two batches [n, h, w, c]."""
    return combine([pair_scales(a, b) for a, b in zip(img1, img2)])
