"""What the seven sample-quality evaluators (frechet.py, manifold.py, kid.py, msssim.py, neighbours.py, swd.py, spectrum.py) have in common: the image and
label layouts they take, one download, the class-grouped feature layout and the classifier handling of the three that read the label
classifier's features, and the stand-alone entry point behind each module's ``main``.  numpy only at import; torch where a function
touches the device."""
import json
import os
import sys

import numpy as np

N_CALIBRATION = 1000


def as_nhwc(images):
    """[n,3072] CHW rows (the data set's layout) or [n,32,32,3] -> [n,32,32,3]."""
    x = np.asarray(images)
    if x.ndim == 2 and x.shape[1] == 3072:
        x = x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    return x


def permuted_labels(labels, confusion_matrix):
    """rcgan-u: conditioning labels mapped through the arg-max permutation of the learned matrix, exactly as
    eval_cifar.generated_label_accuracy maps them."""
    labels = np.asarray(labels)
    cm = np.asarray(confusion_matrix)
    perm = np.zeros_like(cm, dtype=int)
    perm[np.arange(cm.shape[0]), np.argmax(cm, axis=-1)] = 1
    onehot = np.zeros([labels.shape[0], cm.shape[0]], dtype=float)
    onehot[np.arange(labels.shape[0]), labels] = 1
    return np.argmax(onehot.dot(perm), axis=-1)


def check_rows(x, off, what):
    """x: contiguous fp32 [n,d]; off: contiguous int32 [n_seg + 1] -- what every segmented kernel call takes."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("%s: expected contiguous fp32 [n,d], got %s %s" % (what, tuple(x.shape), x.dtype))
    if off.dtype != torch.int32 or off.dim() != 1 or off.numel() < 2 or not off.is_contiguous():
        raise ValueError("%s offsets: expected int32 [n_seg + 1], got %s %s" % (what, tuple(off.shape), off.dtype))


def download(ctx, *tensors):
    """Device tensors -> numpy after ONE synchronisation of the context's stream: the array of one tensor, the list of several."""
    import torch
    with torch.cuda.stream(ctx.stream):
        host = [t.cpu() for t in tensors]
    ctx.stream.synchronize()
    host = [h.numpy() for h in host]
    return host[0] if len(host) == 1 else host


class FeatureSet:
    """One image set's features on the device, twice: in original order as one segment (pooled) and grouped by class with the classes'
    offsets; rows whose label is outside [0, K) are dropped and counted."""

    def __init__(self, ctx, features, labels, n_classes):
        import torch
        f = np.ascontiguousarray(features, np.float32)
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        if f.ndim != 2 or len(lab) != len(f):
            raise ValueError("FeatureSet: features %s, %d labels" % (f.shape, len(lab)))
        ok = (lab >= 0) & (lab < n_classes)
        self.rejected = int((~ok).sum())
        f, lab = f[ok], lab[ok]
        self.n, self.d = f.shape
        if self.n < 1:
            raise ValueError("FeatureSet: no row has a label in [0, %d)" % n_classes)
        order = np.argsort(lab, kind="stable")
        self.count = np.bincount(lab, minlength=n_classes)
        self.off_pooled = np.array([0, self.n], np.int64)
        self.off_grouped = np.concatenate([[0], np.cumsum(self.count)]).astype(np.int64)
        self.ctx = ctx
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
        with torch.cuda.stream(ctx.stream):
            self.pooled, self.grouped = up(f), up(f[order])
            self.d_off_pooled, self.d_off_grouped = up(self.off_pooled.astype(np.int32)), up(self.off_grouped.astype(np.int32))


class FeatureEvaluator:
    """The part of an evaluator that reads the label classifier's frozen features (eval_cifar.LabelClassifier; its class count need
    not be the run's -- only the 64-wide feature is used): a classifier of its own, built from ``asset`` and closed by ``close``,
    unless ``clf`` hands one over, which stays the caller's to close -- several evaluators then read the same features under one
    calibration."""

    def __init__(self, n_classes, asset=None, device=0, chunk=1000, clf=None):
        from .eval_cifar import ASSET, LabelClassifier
        self.asset = ASSET if asset is None else asset
        self.n_classes, self.chunk = int(n_classes), int(chunk)
        self.owns_clf = clf is None
        self.clf = LabelClassifier(device, asset=self.asset) if clf is None else clf
        self.real = None

    def calibrate(self, x, n_calibration=N_CALIBRATION):
        """Calibration on the first n_calibration images; a classifier handed over already calibrated keeps its calibration."""
        if self.owns_clf or self.clf.calibration() is None:
            self.clf.calibrate(x[:n_calibration])

    def feature_set(self, images, labels):
        return FeatureSet(self.clf.ctx, self.clf.features(as_nhwc(images), chunk=self.chunk), labels, self.n_classes)

    def close(self):
        if self.owns_clf:
            self.clf.close()


def standalone(argv, sets, extra, build, json_ready, features=False, evaluate=lambda ev, FLAGS, x, y: ev.evaluate(x, y)):
    """The stand-alone entry point of an evaluator module.  sets: ((flag, what the file is), ...) -- the .npz files (``images``,
    ``labels``) in the order ``prepare_real`` takes them, the set to score last; extra: the module's own (integer flag, default,
    help); features: it takes --label_classifier; build(K, FLAGS, device) -> the evaluator.  Prints the result as one JSON line."""
    from .host import Flags
    f = Flags()
    for name, what in sets:
        f.DEFINE_string(name, None, ".npz with images, labels: " + what)
    if features:
        f.DEFINE_string("label_classifier", None, "weight asset of the feature network; default: the built-in CIFAR-10 network")
    f.DEFINE_integer("n_classes", 0, "class count of the labels; 0: the largest label of %s + 1" % ("either file" if len(sets) == 2 else "the files"))
    for name, default, text in extra:
        f.DEFINE_integer(name, default, text)
    FLAGS = f.parse(sys.argv[1:] if argv is None else argv)
    names = [name for name, _ in sets]
    if any(getattr(FLAGS, name) is None for name in names):
        raise ValueError("flags %s and %s are required" % (", ".join(names[:-1]), names[-1]))
    loaded = []
    for name in names:
        with np.load(getattr(FLAGS, name)) as z:
            loaded.append((z["images"], z["labels"]))
    K = FLAGS.n_classes if FLAGS.n_classes > 0 else int(max(y.max() for _, y in loaded)) + 1
    ev = build(K, FLAGS, int(os.environ.get("LOCAL_RANK", "0")))
    try:
        ev.prepare_real(*[a for s in loaded[:-1] for a in s])
        result = json_ready(evaluate(ev, FLAGS, *loaded[-1]))
    finally:
        ev.close()
    print(json.dumps(result))
    return result
