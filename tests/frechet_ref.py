"""Float64 restatement of the Frechet metric for the tests: the label classifier's forward pass under FROZEN batch-norm statistics
(built on tests/classifier_ref.py's convolution and shortcut), the calibration pass that takes those statistics, two-pass float64
moments, per-class float64 sums with the absolute sums the device kernel's error bound is stated in, and the distance by another
route than the product's (the eigenvalues of the plain product S1 S2 instead of the symmetric S1^1/2 S2 S1^1/2).
The product never imports this module."""
import numpy as np
import torch

from tests import classifier_ref as CR


def load_asset(path, dtype=torch.float64):
    """The float arrays of a weight asset under classifier_ref's names ('|'-separated)."""
    with np.load(path) as z:
        return {k: torch.as_tensor(np.asarray(z[k], np.float64)).to(dtype) for k in z.files if z[k].dtype.kind == "f" and z[k].ndim > 0}


def _forward(P, images_nhwc, bn):
    """The network up to the pooled [n,64] feature; bn(x, name) -> normalised + ReLU."""
    x = torch.as_tensor(np.asarray(images_nhwc), dtype=torch.float64).permute(0, 3, 1, 2)
    h = bn(CR._conv(x, P["conv0|conv"], 1), "conv0")
    for s in range(1, CR.STAGES + 1):
        for b in range(CR.BLOCKS):
            p = "conv%d_%d" % (s, b)
            down = b == 0 and s > 1
            t = h if (s == 1 and b == 0) else bn(h, p + "|conv1_in_block")
            c1 = CR._conv(t, P[p + "|conv1_in_block|conv"], 2 if down else 1)
            c2 = CR._conv(bn(c1, p + "|conv2_in_block"), P[p + "|conv2_in_block|conv"], 1)
            h = c2 + (CR.shortcut_a(h) if down else h)
    return bn(h, "fc").mean(dim=(2, 3))


def _affine_relu(x, P, name, mean, var, eps):
    g, b = P[name + "|gamma"].view(1, -1, 1, 1), P[name + "|beta"].view(1, -1, 1, 1)
    return torch.relu((x - mean.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + eps) * g + b)


def calibrate(P, images_nhwc, eps=CR.BN_EPS):
    """One batch-moment pass -> ({name: (mean, biased variance)} for the 31 layers, the batch-moment features [n,64])."""
    stats = {}

    def bn(x, name):
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        stats[name] = (mean, var)
        return _affine_relu(x, P, name, mean, var, eps)
    with torch.no_grad():
        feat = _forward(P, images_nhwc, bn)
    return stats, feat.numpy()


def features(P, stats, images_nhwc, eps=CR.BN_EPS, chunk=256):
    """Frozen-statistics features [n,64] float64 (chunked only to bound memory: a row does not depend on its batch)."""
    bn = lambda x, name: _affine_relu(x, P, name, stats[name][0], stats[name][1], eps)
    out = []
    with torch.no_grad():
        for lo in range(0, len(images_nhwc), chunk):
            out.append(_forward(P, images_nhwc[lo:lo + chunk], bn).numpy())
    return np.concatenate(out, axis=0)


def moments(x):
    """Two-pass float64 (mean, unbiased covariance) of the rows of x."""
    x = np.asarray(x, np.float64)
    m = x.mean(0)
    c = (x - m).T.dot(x - m) / (len(x) - 1.0)
    return m, c


def class_sums(x, labels, n_classes):
    """Float64 (count [K], sum [K,d], sumsq [K,d,d], rejected) of fp32 rows, per class -- and the absolute sums |x|, |x x^T| the
    error bound of the device accumulation is stated in."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    count, s, ss = np.zeros(n_classes), np.zeros((n_classes, d)), np.zeros((n_classes, d, d))
    sa, ssa = np.zeros((n_classes, d)), np.zeros((n_classes, d, d))
    for k in range(n_classes):
        xs = x[lab == k]
        if len(xs):
            count[k], s[k], ss[k] = len(xs), xs.sum(0), xs.T.dot(xs)
            sa[k], ssa[k] = np.abs(xs).sum(0), np.abs(xs).T.dot(np.abs(xs))
    return count, s, ss, int(((lab < 0) | (lab >= n_classes)).sum()), sa, ssa


def frechet_distance(m1, S1, m2, S2):
    """|m1 - m2|^2 + tr S1 + tr S2 - 2 sum sqrt(eig(S1 S2)), the eigenvalues of the (non-symmetric) product, real parts clipped at 0."""
    ev = np.linalg.eigvals(np.asarray(S1, np.float64).dot(np.asarray(S2, np.float64)))
    tr = np.sqrt(np.clip(ev.real, 0.0, None)).sum()
    d = np.asarray(m1, np.float64) - np.asarray(m2, np.float64)
    return float(d.dot(d) + np.trace(S1) + np.trace(S2) - 2.0 * tr)
