"""Host-side data + label-noise pipeline of the CIFAR engine (product code; numpy legacy RNG so the
label streams are bit-identical to the reference's for the same seed).

Mirrors /root/reference cifar10/common/data/cifar10.py:12-52 (unpickle, cifar_generator, load) and the
two infinite generators of cifar10/gan_resnet.py:864-885.
"""
import os
import pickle

import numpy as np


def C_ALPHA(alpha, n_classes=10):
    """One-coin confusion matrix (gan_resnet.py:106): alpha on the diagonal, (1 - alpha) / (K - 1) off it."""
    K = n_classes
    return ((1 - alpha) / float(K - 1)) * np.ones((K, K)) + (alpha - (1 - alpha) / float(K - 1)) * np.eye(K)


def unpickle(file):
    with open(file, 'rb') as fo:
        d = pickle.load(fo, encoding='bytes')
    return d[b'data'], d[b'labels']


def corrupt_labels(labels, C, rng=np.random, n_classes=None):
    """cifar10.py:29-41: the noisy channel applied to the real labels, the uniformly random generator labels,
    their channel-corrupted version and the C^-1 rows for the unbiased loss.  Draw order is the reference's:
    randint(K, 50000) first, then per sample multinomial(C[label]) and multinomial(C[random]).  K = n_classes, or C's size."""
    K = int(n_classes) if n_classes is not None else len(C)
    if np.shape(C) != (K, K):
        raise ValueError("C has shape %s, expected (%d, %d)" % (np.shape(C), K, K))
    labels = np.array(labels)
    labels_random = rng.randint(K, size=50000)
    labels_biased = np.zeros((50000,))
    labels_inv_weights = np.zeros((50000, K))
    C_inv = np.linalg.inv(C)
    for i in range(len(labels)):
        labels[i] = np.flatnonzero(rng.multinomial(1, C[labels[i], :]))[0]
        labels_inv_weights[i] = C_inv[labels[i], :]
        labels_biased[i] = np.flatnonzero(rng.multinomial(1, C[labels_random[i], :]))[0]
    return labels, labels_random, labels_biased, labels_inv_weights


def check_confusion_matrix(C, n_classes=None):
    """C as a float64 [K,K] row-stochastic matrix (C[y, y~] = P(noisy y~ | clean y)): entries >= 0, rows summing to 1 within 1e-6."""
    C = np.asarray(C, np.float64)
    K = int(n_classes) if n_classes is not None else len(C)
    if C.shape != (K, K):
        raise ValueError("confusion matrix has shape %s, expected (%d, %d)" % (C.shape, K, K))
    if not np.isfinite(C).all() or C.min() < 0:
        raise ValueError("confusion matrix has negative or non-finite entries")
    if np.abs(C.sum(1) - 1.0).max() > 1e-6:
        raise ValueError("confusion matrix rows do not sum to 1 (worst %.3e off)" % np.abs(C.sum(1) - 1.0).max())
    return C


def noisy_labels(labels, C, rs):
    """The noisy channel on a label array, vectorised: one uniform draw per label from ``rs`` (a numpy RandomState), pushed through the
    inverse CDF of C[label].  An entry of probability zero is never drawn.  (``corrupt_labels`` keeps the reference's draw order for
    the GAN trainers; this one serves the label classifier, which has no stream to stay compatible with.)"""
    labels = np.asarray(labels, np.int64)
    C = check_confusion_matrix(C)
    if labels.size and (labels.min() < 0 or labels.max() >= len(C)):
        raise ValueError("labels outside [0, %d)" % len(C))
    cdf = np.cumsum(C, axis=1)
    cdf /= cdf[:, -1:]                                   # the last entry exactly 1: a draw u < 1 never runs off the end
    u = rs.random_sample(labels.shape[0])
    return (u[:, None] >= cdf[labels]).sum(axis=1).astype(np.int64)


def estimate_confusion_anchor(probs, quantile=0.97):
    """Patrini et al. 2017, eq. 12-13: row i of the estimate is the noisy-label posterior ``probs`` [N,K] at the sample that sits at
    ``quantile`` of column i (the sample the classifier is surest belongs to class i; a quantile below 1 guards against outliers).
    quantile = 1.0 takes the arg-max sample, the lowest index on ties.  The rows are the samples' own probabilities, untouched: they
    sum to 1 as well as ``probs`` does."""
    probs = np.asarray(probs, np.float64)
    if probs.ndim != 2 or probs.shape[0] < 1:
        raise ValueError("probs has shape %s, expected [N, K]" % (probs.shape,))
    if not 0.0 < quantile <= 1.0:
        raise ValueError("quantile %r outside (0, 1]" % (quantile,))
    n, K = probs.shape
    C = np.zeros((K, K))
    for i in range(K):
        if quantile >= 1.0:
            at = int(np.argmax(probs[:, i]))
        else:
            # the sample whose column-i probability is nearest the quantile from below (numpy's "lower" rule), lowest index on ties
            order = np.argsort(probs[:, i], kind="stable")
            at = int(order[int(np.floor(quantile * (n - 1)))])
        C[i] = probs[at]
    return C


def cifar_generator(images, labels, batch_size, C, rng=np.random):
    """cifar10.py:19-45 on in-memory arrays: fixed order, no shuffling, tail dropped.  The class count is C's size."""
    labels, labels_random, labels_biased, labels_inv_weights = corrupt_labels(labels, C, rng)

    def get_epoch():
        for i in range(int(len(images) / batch_size)):
            s = slice(i * batch_size, (i + 1) * batch_size)
            yield (images[s], labels[s], labels_random[s], labels_biased[s], labels_inv_weights[s])
    return get_epoch


def load(batch_size, data_dir, C, rng=np.random):
    """cifar10.py:48-52."""
    def read(files):
        xs, ys = [], []
        for f in files:
            x, y = unpickle(os.path.join(data_dir, f))
            xs.append(x)
            ys.append(y)
        return np.concatenate(xs, axis=0), np.concatenate(ys, axis=0)
    tx, ty = read(['data_batch_%d' % i for i in range(1, 6)])
    vx, vy = read(['test_batch'])
    return cifar_generator(tx, ty, batch_size, C, rng), cifar_generator(vx, vy, batch_size, C, rng)


def unpickle100(file, coarse=False):
    """A cifar-100-python pickle ("train" / "test"): images [n,3072] and the 100 fine labels, or the 20 coarse ones."""
    with open(file, 'rb') as fo:
        d = pickle.load(fo, encoding='bytes')
    return d[b'data'], d[b'coarse_labels' if coarse else b'fine_labels']


def load100(batch_size, data_dir, C, rng=np.random, coarse=False):
    """``load`` for CIFAR-100 (data_dir = the cifar-100-python directory): 100 fine classes, or 20 coarse ones with coarse=True.
    C is the [K, K] confusion matrix of that class count."""
    K = 20 if coarse else 100
    if np.shape(C) != (K, K):
        raise ValueError("CIFAR-100 with %s labels has %d classes; C has shape %s" % ("coarse" if coarse else "fine", K, np.shape(C)))
    tx, ty = unpickle100(os.path.join(data_dir, 'train'), coarse)
    vx, vy = unpickle100(os.path.join(data_dir, 'test'), coarse)
    return cifar_generator(np.asarray(tx), np.asarray(ty), batch_size, C, rng), cifar_generator(np.asarray(vx), np.asarray(vy), batch_size, C, rng)


def class_templates(n_classes=10):
    """Fixed low-frequency colour patterns [K,3,32,32] (sums of three separable cosines per channel, frequencies 0..2):
    the class-carrying part of the "templates" synthetic images.  Not reference data -- a stand-in for CIFAR-10 (no dataset and
    no network here) on which a generated image's class can be read off exactly (eval_cifar.TemplateClassifier).  The first ten
    patterns are the same for every K (one stream, drawn class after class)."""
    trs = np.random.RandomState(4242)
    yy, xx = np.mgrid[0:32, 0:32] / 32.0
    tmpl = np.zeros((n_classes, 3, 32, 32))
    for c in range(n_classes):
        for ch in range(3):
            for _ in range(3):
                fx, fy = trs.randint(0, 3, size=2)
                px, py = trs.uniform(0, 2 * np.pi, size=2)
                tmpl[c, ch] += trs.uniform(0.3, 1.0) * np.cos(2 * np.pi * fx * xx + px) * np.cos(2 * np.pi * fy * yy + py)
    return tmpl


def template_images(rs, labels, n_classes=10):
    """uint8-valued CHW rows [n,3072]: tanh(0.6 template[label] + 0.6 low-pass noise) mapped to 0..255 -- natural-image-like
    second-order statistics that carry the label (per-image noise sigma ~ 1.4 pixels, as strong as the class pattern)."""
    n = len(labels)
    noise = rs.randn(n, 3, 32, 32)
    for _ in range(4):          # separable [1 2 1]/4 blur, wrap-around
        noise = (np.roll(noise, 1, 2) + 2 * noise + np.roll(noise, -1, 2)) / 4
        noise = (np.roll(noise, 1, 3) + 2 * noise + np.roll(noise, -1, 3)) / 4
    noise /= noise.std()
    img = np.tanh(0.6 * class_templates(n_classes)[np.asarray(labels)] + 0.6 * noise)
    return np.clip(np.floor((img * 0.5 + 0.5) * 256.0), 0, 255).astype(np.int64).reshape(n, 3072)


def synthetic_cifar(n=50000, seed=1234, kind="uniform", n_classes=10):
    """Synthetic stand-ins for the CIFAR arrays.  kind "uniform" (SURVEY 8(d)): uint8 images U{0..255} [n,3072] (CHW) and
    clean labels U{0..K-1} -- timing / plumbing only, the images carry no label.  kind "templates": ``template_images`` of the
    clean labels -- a learnable conditional distribution for end-to-end training runs."""
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        return rs.randint(0, 256, size=(n, 3072), dtype=np.uint8), rs.randint(n_classes, size=n)
    if kind != "templates":
        raise ValueError("unknown synthetic kind %r" % (kind,))
    labels = rs.randint(n_classes, size=n)
    images = np.concatenate([template_images(rs, labels[i:i + 5000], n_classes) for i in range(0, n, 5000)]).astype(np.uint8)
    return images, labels


def inf_train_gen(train_gen):
    """gan_resnet.py:865-868."""
    while True:
        for batch in train_gen():
            yield batch


def inf_train_gen_G(train_gen, gen_bs_multiple=2):
    """gan_resnet.py:869-882: generator labels = consecutive (random, biased) batches of a second pass."""
    it = train_gen()
    while True:
        rnd, bia = [], []
        for _ in range(gen_bs_multiple):
            try:
                _, _, r, b, _ = next(it)
            except StopIteration:
                it = train_gen()
                _, _, r, b, _ = next(it)
            rnd.append(r)
            bia.append(b)
        yield np.concatenate(rnd, axis=0), np.concatenate(bia, axis=0)
