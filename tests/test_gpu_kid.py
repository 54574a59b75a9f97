"""The kernel distance on the GPU: KernelDistanceEvaluator on the classifier's frozen features of template images against the
brute-force float64 restatement (tests/kid_ref.py) on the same, downloaded, features; the orderings the numbers exist for; the
training command line.

Agreement is within the kernel's derived row bounds (tests/test_gpu_ksum.py) carried through the estimator.  With b_gg, b_rr, b_gr
the sums of the row bounds of a segment's three row-sum vectors, the estimate S_gg / (m (m-1)) + S_rr / (n (n-1)) - 2 S_gr / (m n)
moves by at most b_gg / (m (m-1)) + b_rr / (n (n-1)) + 2 b_gr / (m n), plus 1e-12 of the sum of the three terms' magnitudes for the
float64 sums the host takes in another order than the restatement.  A mean over segments moves by at most the largest segment
allowance; so does a standard deviation over them (ddof 0), and a standard error std(ddof 1) / sqrt(K) by at most that / sqrt(K - 1)."""
import os
import re

import numpy as np
import pytest

from tests import kid_ref as KR
from tests.train_launch import launch as _launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, K, SUBSET, N_CALIB = 512, 10, 128, 128
ROUNDING = 1e-12


def _templates(seed, n, classes=10):
    """n template images (NHWC raw pixels) with labels uniform over the first ``classes`` classes."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as DT
    rs = np.random.RandomState(seed)
    labels = rs.randint(classes, size=n)
    x = DT.template_images(rs, labels).reshape(n, 3, 32, 32).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(x), labels


def _allowance(g, r):
    """How far the estimate of one segment may move (see above); 0 for a segment that is left out."""
    m, n = len(g), len(r)
    if m < 2 or n < 2:
        return 0.0
    gamma = KR.gamma_of(g.shape[1])
    b_gg = KR.row_bound(g, g, gamma, 1.0, np.eye(m, dtype=bool))[0].sum()
    b_rr = KR.row_bound(r, r, gamma, 1.0, np.eye(n, dtype=bool))[0].sum()
    b_gr = KR.row_bound(g, r, gamma, 1.0)[0].sum()
    Kgg, Krr, Kgr = KR.kernel(g, g), KR.kernel(r, r), KR.kernel(g, r)
    size = (np.abs(Kgg).sum() - np.abs(np.diag(Kgg)).sum()) / (m * (m - 1.0)) + (np.abs(Krr).sum() - np.abs(np.diag(Krr)).sum()) / (n * (n - 1.0)) \
        + 2.0 * np.abs(Kgr).sum() / (m * float(n))
    return float(b_gg / (m * (m - 1.0)) + b_rr / (n * (n - 1.0)) + 2.0 * b_gr / (m * float(n)) + ROUNDING * size)


@pytest.fixture(scope="module")
def world():
    """One classifier calibrated on 128 template images; set A (real) and set B (generated): two draws of one distribution, 512
    images each; their features, downloaded once; one evaluator with A prepared; the reference's result, computed once."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import kid as KD
    from rcgan_amd.eval_cifar import LabelClassifier
    clf = LabelClassifier(0, arena_bytes=2 << 30)
    calib, _ = _templates(21, N_CALIB)
    (xa, la), (xb, lb) = _templates(22, N), _templates(23, N)
    clf.calibrate(calib)
    ev = KD.KernelDistanceEvaluator(K, subset_size=SUBSET, chunk=256, clf=clf)
    ev.prepare_real(xa, la)                       # (the classifier arrives calibrated: its calibration is kept)
    fa, fb = clf.features(xa, chunk=256), clf.features(xb, chunk=256)
    w = dict(KD=KD, clf=clf, ev=ev, xa=xa, la=la, xb=xb, lb=lb, fa=fa, fb=fb, ref=KR.evaluate(fa, la, fb, lb, K, SUBSET),
             got=ev.evaluate(xb, lb))
    yield w
    ev.close()                                    # (does not own the classifier)
    clf.close()


def test_the_evaluator_agrees_with_the_float64_restatement_on_its_own_features(world):
    w = world
    got, ref, fa, la, fb, lb = w["got"], w["ref"], w["fa"], w["la"], w["fb"], w["lb"]
    assert fa.shape == (N, 64) and fa.dtype == np.float32
    pooled = _allowance(fb, fa)
    per = np.array([_allowance(fb[lb == c], fa[la == c]) for c in range(K)])
    subs = np.array([_allowance(fb[b * SUBSET:(b + 1) * SUBSET], fa[b * SUBSET:(b + 1) * SUBSET]) for b in range(N // SUBSET)])
    print("kernel_distance %.6e (reference %.6e, allowance %.2e); intra-class %.6e +- %.2e (allowance %.2e); subsets %.6e +- %.2e"
          % (got["kernel_distance"], ref["kernel_distance"], pooled, got["intra_class_kernel_distance"], got["intra_class_kernel_distance_se"],
             per.max(), got["subset_mean"], got["subset_std"]))
    assert abs(got["kernel_distance"] - ref["kernel_distance"]) <= pooled
    assert got["classes_used"] == ref["classes_used"] == K and got["left_out"] == ref["left_out"] == []
    assert (np.abs(got["per_class"] - ref["per_class"]) <= per).all()
    assert abs(got["intra_class_kernel_distance"] - ref["intra_class_kernel_distance"]) <= per.max()
    assert abs(got["intra_class_kernel_distance_se"] - ref["intra_class_kernel_distance_se"]) <= per.max() / np.sqrt(K - 1.0)
    assert got["subsets"] == ref["subsets"] == N // SUBSET
    assert abs(got["subset_mean"] - ref["subset_mean"]) <= subs.max() and abs(got["subset_std"] - ref["subset_std"]) <= subs.max()
    assert (got["rejected_real"], got["rejected_generated"]) == (0, 0)


def test_shifted_labels_leave_the_pooled_and_subset_numbers_alone_and_raise_the_intra_class_distance(world):
    w = world
    shifted = (w["lb"] + 1) % K                   # every generated image carries the label of another class
    for name, clean, mixed in (("reference", w["ref"], KR.evaluate(w["fa"], w["la"], w["fb"], shifted, K, SUBSET)),
                               ("engine", w["got"], w["ev"].evaluate(w["xb"], shifted))):
        print("%s: intra-class kernel distance clean %.5f, labels shifted %.5f" % (name, clean["intra_class_kernel_distance"],
                                                                                  mixed["intra_class_kernel_distance"]))
        for key in ("kernel_distance", "subset_mean", "subset_std"):
            assert np.float64(mixed[key]).tobytes() == np.float64(clean[key]).tobytes(), (name, key)      # they cannot see the labels
        assert mixed["subsets"] == clean["subsets"]
        assert mixed["intra_class_kernel_distance"] > clean["intra_class_kernel_distance"], name


def test_a_set_of_half_the_classes_is_further_away_and_the_absent_classes_are_left_out(world):
    w = world
    xh, lh = _templates(24, N, classes=5)         # classes 0-4 only
    half = w["ev"].evaluate(xh, lh)
    print("pooled kernel distance: independent full draw %.5f, classes 0-4 only %.5f" % (w["got"]["kernel_distance"], half["kernel_distance"]))
    assert half["kernel_distance"] > w["got"]["kernel_distance"] and half["kernel_distance"] > 0
    assert half["left_out"] == [5, 6, 7, 8, 9] and half["classes_used"] == 5
    assert np.isnan(half["per_class"][5:]).all() and not np.isnan(half["per_class"][:5]).any()
    # absent on the REAL side: the same
    ev = w["KD"].KernelDistanceEvaluator(K, subset_size=SUBSET, chunk=256, clf=w["clf"])
    keep = w["la"] != 3
    ev.prepare_real(w["xa"][keep], w["la"][keep])
    r = ev.evaluate(w["xb"], w["lb"])
    assert r["left_out"] == [3] and r["classes_used"] == K - 1 and np.isnan(r["per_class"][3])
    assert r["rejected_real"] == 0 and r["subsets"] == int(keep.sum()) // SUBSET


# ------------------------------------------------------------------------------------------------------------- command line
LINES = ["kernel_distance", "intra_class_kernel_distance", "kernel_distance_subsets"]
PRDC = ["--prdc_freq", "2", "--prdc_samples", "512", "--prdc_real_samples", "1024"]
KID = ["--kid_freq", "2", "--kid_samples", "512", "--kid_real_samples", "1024", "--kid_subset_size", "128"]


def test_training_logs_the_three_lines_at_every_period_and_at_the_end_with_one_classifier(tmp_path):
    text, built = _launch(tmp_path, PRDC + KID, "k1")
    num = r"(-?[\d.]+(?:e[-+]?\d+)?|nan)"
    pooled = re.findall(r"INFO\s+kernel_distance: %s$" % num, text, flags=re.M)
    intra = re.findall(r"INFO\s+intra_class_kernel_distance: %s \+- %s \((\d+) of 10 classes\)$" % (num, num), text, flags=re.M)
    subs = re.findall(r"INFO\s+kernel_distance_subsets: %s \+- %s \((\d+) of size 128\)$" % (num, num), text, flags=re.M)
    assert len(pooled) == len(intra) == len(subs) == 3, text[-3000:]              # iterations 2 and 4, and the end of training
    assert all(np.isfinite(float(v)) for v in pooled)
    assert all(np.isfinite(float(a)) and float(b) >= 0 and int(c) == 10 for a, b, c in intra)
    assert all(np.isfinite(float(a)) and float(b) >= 0 and int(c) == 3 for a, b, c in subs)          # (500 generated rows: 3 subsets of 128)
    assert "kernel distance real set: 1024 images, label classifier shared" in text
    assert "manifold_precision" in text
    assert built == 1


def test_the_same_command_without_the_flag_logs_none_of_them(tmp_path):
    text, built = _launch(tmp_path, PRDC, "k0")
    assert "kernel_distance" not in text and "kernel distance" not in text and built == 1
    assert "manifold_precision" in text
