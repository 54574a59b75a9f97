"""Record tests/golden/ref_msssim.npz: small uint8 inputs with the outputs of the reference's cifar10/common/msssim.py on them.

    python tests/tools/record_msssim_golden.py /path/to/reference [out.npz]

The reference's module is imported by path with a stand-in for the ``tensorflow`` flags it defines at import (nothing else of
tensorflow is touched by the two functions called here).  Per shape (32x32x3, 28x28x1, 16x16x1, 17x23x3) the file holds
  images_<shape>  uint8 [n,h,w,c]: template images of two classes (crops / one channel for the smaller shapes) and one image plus noise
  pairs_<shape>   int32 [P,2]
  scales_<shape>  float64 [P,2,5]: per pair and level, row 0 the cs and row 1 the ssim that _SSIMForMultiScale returns for the batch of
                  that one pair; the level's inputs are the 2 x 2 means of tests/msssim_ref.py (dyadic numbers, exact in float64)
  value_<shape>   MultiScaleSSIM of the batch of all P pairs (which walks the levels with the reference's own down-sampling)
and ``noise_images`` / ``noise_pairs`` / ``noise_value``: a batch of 8 pairs of uniform-noise images on which MultiScaleSSIM is nan.
Every structured batch is checked to be finite here."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = ((32, 32, 3), (28, 28, 1), (16, 16, 1), (17, 23, 3))


def load_reference(ref_root):
    flags = types.SimpleNamespace(DEFINE_string=lambda *a, **k: None, FLAGS=types.SimpleNamespace())
    sys.modules.setdefault("tensorflow", types.SimpleNamespace(flags=flags))
    spec = importlib.util.spec_from_file_location("reference_msssim", os.path.join(ref_root, "cifar10", "common", "msssim.py"))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def inputs(shape, seed):
    """8 images: three templates of class 0, three of class 1, the first image plus noise of sigma 8 and of sigma 40."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as DT
    h, w, c = shape
    rs = np.random.RandomState(seed)
    x = DT.template_images(rs, np.array([0, 0, 0, 1, 1, 1])).reshape(6, 3, 32, 32).transpose(0, 2, 3, 1)
    x = x[:, (32 - h) // 2:(32 - h) // 2 + h, (32 - w) // 2:(32 - w) // 2 + w, :c].astype(np.float64)
    noisy = [np.clip(np.rint(x[0] + s * rs.randn(h, w, c)), 0, 255) for s in (8.0, 40.0)]
    images = np.concatenate([x, np.stack(noisy)]).astype(np.uint8)
    pairs = np.array([(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (0, 6), (0, 7), (2, 2), (1, 3)], np.int32)
    return images, pairs


def main(argv):
    from tests import msssim_ref as MR
    ref = load_reference(argv[0])
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_msssim.npz")
    out = {}
    for k, shape in enumerate(SHAPES):
        tag = "%dx%dx%d" % shape
        images, pairs = inputs(shape, 100 + k)
        scales = np.zeros((len(pairs), 2, 5))
        for p, (i, j) in enumerate(pairs):
            a, b = images[i].astype(np.float64), images[j].astype(np.float64)
            for l in range(5):
                scales[p, 1, l], scales[p, 0, l] = ref._SSIMForMultiScale(a[None], b[None], max_val=255)
                a, b = MR._half(a), MR._half(b)
        value = float(ref.MultiScaleSSIM(images[pairs[:, 0]], images[pairs[:, 1]], max_val=255))
        assert np.isfinite(scales).all() and np.isfinite(value), tag
        print("%s: MultiScaleSSIM of %d pairs %.12f" % (tag, len(pairs), value))
        out.update({"images_" + tag: images, "pairs_" + tag: pairs, "scales_" + tag: scales, "value_" + tag: np.float64(value)})
    pairs = np.arange(16, dtype=np.int32).reshape(8, 2)
    for seed in range(1000):                  # the first seed whose batch of 8 noise pairs the reference cannot score
        noise = np.random.RandomState(seed).randint(0, 256, size=(16, 32, 32, 3)).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            value = float(ref.MultiScaleSSIM(noise[pairs[:, 0]], noise[pairs[:, 1]], max_val=255))
        if np.isnan(value):
            break
    assert np.isnan(value)
    print("noise: seed %d gives nan" % seed)
    out.update(noise_images=noise, noise_pairs=pairs, noise_value=np.float64(value))
    np.savez_compressed(out_path, **out)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1:])
