"""The Frechet metric on the GPU: the classifier's frozen-statistics feature pass against its float64 restatement
(tests/frechet_ref.py), the property that pass exists for (a sample's feature does not depend on its batch), the ordering of the
distances on template images, and the training command line."""
import os
import re

import numpy as np
import pytest

from tests import frechet_ref as FRF
from tests.train_launch import launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSET = os.path.join(ROOT, "robust-conditional-gan_amd", "assets", "cifar_label_classifier.npz")

# Frozen-pass features, engine (fp32 on the fp32 matrix cores) vs the float64 restatement: max |error| relative to max |reference|.
# Measured on an MI355X: 3.578e-06 (64 template images under 128 calibration images; 31 convolutions and batch norms whose
# summation order differs; the batch-moment features of the calibration batch: 4.174e-06 under the same bound).  The assertion
# allows four times the measured value.
PARITY_MEASURED = 3.578e-6
PARITY_TOL = 4 * PARITY_MEASURED


def _templates(seed, n, classes=10):
    """n template images (NHWC raw pixels) with labels uniform over the first ``classes`` classes."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    rs = np.random.RandomState(seed)
    labels = rs.randint(classes, size=n)
    x = D.template_images(rs, labels).reshape(n, 3, 32, 32).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(x), labels


@pytest.fixture(scope="module")
def clf():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.eval_cifar import LabelClassifier
    c = LabelClassifier(0, arena_bytes=2 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parity(clf):
    """Calibration on 128 template images, engine and restatement, computed once."""
    P = FRF.load_asset(ASSET)
    calib, _ = _templates(11, 128)
    others, _ = _templates(12, 64)
    batch_feat = clf.calibrate(calib)
    stats, ref_batch_feat = FRF.calibrate(P, calib)
    return dict(P=P, calib=calib, others=others, stats=stats, batch_feat=batch_feat, ref_batch_feat=ref_batch_feat,
                pairs=clf.calibration())


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def test_frozen_features_match_the_float64_restatement(clf, parity):
    from rcgan_amd.eval_cifar import bn_layer_names
    clf.set_calibration(parity["pairs"])
    got = clf.features(parity["others"])
    ref = FRF.features(parity["P"], parity["stats"], parity["others"])
    assert got.shape == (64, 64) and got.dtype == np.float32
    err = _rel(got, ref)
    print("frozen features vs float64: max err / max|ref| = %.3e" % err)
    # the calibration pairs themselves: 31 layers, mean and biased variance
    assert list(parity["pairs"]) == bn_layer_names() and len(parity["pairs"]) == 31
    worst = 0.0
    for k in bn_layer_names():
        m, v = parity["stats"][k.replace("/", "|")]
        worst = max(worst, _rel(parity["pairs"][k][0], m.numpy()), _rel(parity["pairs"][k][1], v.numpy()))
    print("calibration pairs vs float64: worst max err / max|ref| = %.3e" % worst)
    assert err <= PARITY_TOL, err
    # chunking, a tail chunk included, changes fp32 rounding at the most (a convolution may take another route at another batch size)
    assert _rel(clf.features(parity["others"], chunk=24), got.astype(np.float64)) <= PARITY_TOL


def test_a_feature_does_not_depend_on_its_batch_bit_for_bit(clf, parity):
    clf.set_calibration(parity["pairs"])
    x = parity["others"][:8]
    alone, together = clf.features(x[:3]), clf.features(x)
    assert np.array_equal(alone, together[:3])
    ref = FRF.features(parity["P"], parity["stats"], x)
    assert np.array_equal(FRF.features(parity["P"], parity["stats"], x[:3]), ref[:3])
    # the batch-moment path on the same two batches does depend on the batch: this test cannot pass by calling that one
    assert not np.array_equal(clf.batch_moment_features(x[:3]), clf.batch_moment_features(x)[:3])


def test_frozen_features_of_the_calibration_batch_equal_its_batch_moment_features(clf, parity):
    clf.set_calibration(parity["pairs"])
    frozen = clf.features(parity["calib"])
    err_engine = _rel(frozen, parity["batch_feat"].astype(np.float64))
    err_ref = _rel(parity["batch_feat"], parity["ref_batch_feat"])
    print("frozen vs batch-moment features of the calibration batch: %.3e; batch-moment vs float64: %.3e" % (err_engine, err_ref))
    assert err_engine <= PARITY_TOL and err_ref <= PARITY_TOL
    assert np.array_equal(clf.batch_moment_features(parity["calib"]), parity["batch_feat"])


def test_features_need_a_calibration():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.eval_cifar import LabelClassifier
    c = LabelClassifier(0, arena_bytes=1 << 28)
    try:
        with pytest.raises(RuntimeError, match="calibrate"):
            c.features(np.zeros((2, 32, 32, 3)))
        assert c.calibration() is None
    finally:
        c.close()


def test_distances_order_template_sets_as_they_should(clf):
    """512 calibration images, 2048 images per set in chunks of 256.  On the float64 restatement with the committed asset: pooled
    A|B 0.148, A|B restricted to classes 0-4 0.356, A|uniform noise 311; per-class mean A|B 1.65, with B's labels shifted by one 3.00."""
    from rcgan_amd import frechet as FR
    n, K = 2048, 10
    calib, _ = _templates(21, 512)
    (xa, la), (xb, lb) = _templates(22, n), _templates(23, n)
    noise = np.random.RandomState(24).randint(0, 256, size=(n, 32, 32, 3))
    clf.calibrate(calib)

    def moments(x, labels):
        mom = FR.ClassMoments(clf.ctx, clf.FEATURE_DIM, K)
        assert clf.features(x, labels, moments=mom, chunk=256) is None
        return mom.download()
    A, B = moments(xa, la), moments(xb, lb)
    half = lb < 5
    same = FR.evaluate(A, B)
    halved = FR.evaluate(A, moments(xb[half], lb[half]))
    noisy = FR.evaluate(A, moments(noise, la))
    shifted = FR.evaluate(A, moments(xb, (lb + 1) % K))
    print("pooled: same %.4f, classes 0-4 %.4f, noise %.2f; per class: clean %.4f, shifted %.4f; smallest class %d"
          % (same["frechet_distance"], halved["frechet_distance"], noisy["frechet_distance"], same["intra_class_frechet_distance"],
             shifted["intra_class_frechet_distance"], int(min(A.count.min(), B.count.min()))))
    assert same["left_out"] == [] and shifted["left_out"] == [] and same["classes_used"] == K
    assert halved["left_out"] == [5, 6, 7, 8, 9]
    assert (same["rejected_real"], same["rejected_generated"]) == (0, 0)
    assert noisy["frechet_distance"] > 100 * same["frechet_distance"]
    assert halved["frechet_distance"] > 1.5 * same["frechet_distance"]
    assert shifted["intra_class_frechet_distance"] > 1.4 * same["intra_class_frechet_distance"]
    assert abs(shifted["frechet_distance"] - same["frechet_distance"]) <= 1e-9 * same["frechet_distance"]      # the pooled one cannot see it
    # kernel + host arithmetic, apart from the network: the restatement's distance on the engine's downloaded features
    fa, fb = clf.features(xa, chunk=256), clf.features(xb, chunk=256)
    want = FRF.frechet_distance(*FRF.moments(fa), *FRF.moments(fb))
    assert abs(same["frechet_distance"] - want) <= 1e-6 * want, (same["frechet_distance"], want)
    for k in (0, 9):
        want_k = FRF.frechet_distance(*FRF.moments(fa[la == k]), *FRF.moments(fb[lb == k]))
        assert abs(same["per_class"][k] - want_k) <= 1e-6 * want_k, k


def test_the_stand_alone_entry_compares_two_sample_dumps(tmp_path, capsys):
    """Two .npz dumps (one as NHWC images, one as the data set's channel-major rows) -> one JSON line with the same numbers."""
    import json
    from rcgan_amd import frechet as FR
    (xa, la), (xb, lb) = _templates(31, 1200), _templates(32, 400)
    a, b = os.path.join(str(tmp_path), "a.npz"), os.path.join(str(tmp_path), "b.npz")
    np.savez(a, images=xa.astype(np.uint8), labels=la)
    np.savez(b, images=xb.transpose(0, 3, 1, 2).reshape(len(xb), 3072).astype(np.uint8), labels=lb)
    capsys.readouterr()
    result = FR.main(["--real", a, "--generated", b])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(result))
    assert line["classes_used"] == 10 and line["left_out"] == [] and len(line["per_class"]) == 10
    assert np.isfinite(line["frechet_distance"]) and 0 <= line["frechet_distance"] < 5      # two draws of one distribution
    assert line["intra_class_frechet_distance"] == pytest.approx(np.mean(line["per_class"]), rel=1e-12)
    # the same numbers through the pieces: calibration on the first 1000 real images, frozen features, host moments
    ev = FR.FrechetEvaluator(10)
    try:
        ev.clf.calibrate(xa[:1000])
        want = FR.evaluate(FR.moments_of(ev.clf.features(xa), la, 10), FR.moments_of(ev.clf.features(xb), lb, 10))
    finally:
        ev.close()
    assert abs(line["frechet_distance"] - want["frechet_distance"]) <= 1e-6 * want["frechet_distance"]
    with pytest.raises(ValueError, match="required"):
        FR.main(["--real", a])


# ------------------------------------------------------------------------------------------------------------- command line
def _launch(tmp_path, extra, expt="f1"):
    """Two iterations through the reference-compatible launcher."""
    return launch(tmp_path, extra, expt, niters=2, script=os.path.join(ROOT, "cifar10", "gan_resnet.py"))[0]


def _logged(text, name):
    """The values of the evaluation's own log lines '<name>: value[ (k of K classes)]' (not the plot summary's 'a: 1, b: 2' lines)."""
    return [float(v) for v in re.findall(r"INFO\s+%s: (\S+)(?: \(\d+ of \d+ classes\))?$" % re.escape(name), text, flags=re.M)]


FRECHET = ["--frechet_freq", "2", "--frechet_samples", "512", "--frechet_real_samples", "1024"]


def test_training_logs_both_distances_writes_the_cache_and_reuses_it(tmp_path):
    cache = os.path.join(str(tmp_path), "f1", "frechet_real_stats.npz")
    text = _launch(tmp_path, FRECHET)
    pooled, intra = _logged(text, "frechet_distance"), _logged(text, "intra_class_frechet_distance")
    assert len(pooled) == len(intra) == 2, text[-3000:]           # iteration 1 and the end of training
    assert all(np.isfinite(v) and v >= 0 for v in pooled + intra)
    assert "(10 of 10 classes)" in text
    assert "frechet real statistics: 1024 images, computed" in text and os.path.exists(cache)
    with np.load(cache) as z:
        assert z["count"].sum() == 1024 and z["mean"].shape == (10, 64) and z["cov"].shape == (10, 64, 64)
        assert len([k for k in z.files if k.startswith("calib_mean_")]) == 31
    mtime = os.stat(cache).st_mtime_ns
    text = _launch(tmp_path, FRECHET)
    assert "frechet real statistics: 1024 images, reused from frechet_real_stats.npz" in text and "images, computed" not in text
    assert os.stat(cache).st_mtime_ns == mtime
    assert len(_logged(text, "frechet_distance")) == 2


def test_without_the_flag_nothing_is_written_or_logged(tmp_path):
    text = _launch(tmp_path, [], expt="f0")
    assert "frechet" not in text
    assert not os.path.exists(os.path.join(str(tmp_path), "f0", "frechet_real_stats.npz"))


def test_the_assets_class_count_is_not_checked_against_the_runs(tmp_path):
    text = _launch(tmp_path, ["--dataset", "cifar100", "--coarse_labels"] + FRECHET, expt="f20")
    pooled, intra = _logged(text, "frechet_distance"), _logged(text, "intra_class_frechet_distance")
    assert len(pooled) == len(intra) == 2 and all(np.isfinite(v) and v >= 0 for v in pooled + intra), text[-3000:]
    assert "(20 of 20 classes)" in text
