"""The Frechet metric without a GPU: the two entry points of csrc/moments.hip are exported and check their arguments before
anything touches a device, the host arithmetic of frechet.py has the closed forms of the distance, ``evaluate`` leaves out what it
must, the pooled moments come out of the per-class sums, and the real set's cache is keyed as it says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import frechet_ref as FRF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fr():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import frechet
    return frechet


def _spd(rs, d, scale=1.0):
    a = rs.randn(d, 2 * d)
    return scale * a.dot(a.T) / (2 * d)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_entry_points_and_check_arguments_without_a_device():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in ("rcgan_class_moments_bytes", "rcgan_class_moments_accum"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    feat = (C.c_float * 256)()
    labels = (C.c_int32 * 4)()
    state = (C.c_double * 4096)()
    for lib in (_lib.load(), _lib.load("f16")):
        call = lambda n, d, K, lab: lib.rcgan_class_moments_accum(None, n, d, K, C.cast(feat, C.c_void_p),
                                                                  C.cast(lab, C.c_void_p) if lab is not None else None,
                                                                  C.cast(state, C.c_void_p))
        assert call(1, 0, 1, labels) == _lib.EINVALID_ARG
        assert call(1, 257, 1, labels) == _lib.EINVALID_ARG
        assert call(1, 4, 0, labels) == _lib.EINVALID_ARG
        assert call(1, 4, 1025, labels) == _lib.EINVALID_ARG
        assert call(1, 4, 2, None) == _lib.EINVALID_ARG
        assert call(0, 4, 2, labels) == _lib.EINVALID_ARG
        assert all(v == 0.0 for v in state)              # nothing was written
        size = lib.rcgan_class_moments_bytes
        assert size(64, 10) == 8 * (10 + 10 * 64 + 10 * 64 * 64 + 1)
        assert size(1, 1) == 8 * 4
        for bad in ((0, 1), (257, 1), (4, 0), (4, 1025)):
            assert size(*bad) == 0, bad
        ds = [size(d, 10) for d in (1, 3, 64, 67, 256)]
        ks = [size(64, k) for k in (1, 2, 10, 17, 1024)]
        assert all(a < b for a, b in zip(ds, ds[1:])) and all(a < b for a, b in zip(ks, ks[1:]))


# ------------------------------------------------------------------------------------------------------------- the distance
def test_equal_inputs_give_zero():
    fr, rs = _fr(), np.random.RandomState(0)
    S, m = _spd(rs, 64), rs.randn(64)
    assert abs(fr.frechet_distance(m, S, m, S)) <= 1e-9


def test_equal_covariance_and_a_mean_shift_give_the_squared_shift():
    fr, rs = _fr(), np.random.RandomState(1)
    S, m, delta = _spd(rs, 64), rs.randn(64), rs.randn(64)
    assert abs(fr.frechet_distance(m, S, m + delta, S) - delta.dot(delta)) <= 1e-9 * delta.dot(delta)


def test_diagonal_covariances_have_the_closed_form():
    fr, rs = _fr(), np.random.RandomState(2)
    a, b = rs.uniform(0.1, 4.0, 64), rs.uniform(0.1, 4.0, 64)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(fr.frechet_distance(np.zeros(64), np.diag(a), np.zeros(64), np.diag(b)) - want) <= 1e-10 * want


def test_the_distance_is_symmetric_in_its_arguments():
    fr, rs = _fr(), np.random.RandomState(3)
    S1, S2, m1, m2 = _spd(rs, 64), _spd(rs, 64, 3.0), rs.randn(64), rs.randn(64)
    a, b = fr.frechet_distance(m1, S1, m2, S2), fr.frechet_distance(m2, S2, m1, S1)
    assert abs(a - b) <= 1e-10 * a
    assert abs(a - FRF.frechet_distance(m1, S1, m2, S2)) <= 1e-9 * a          # the restatement's route: eigenvalues of S1 S2


def test_rank_deficient_covariances_give_a_finite_non_negative_number():
    fr, rs = _fr(), np.random.RandomState(4)
    x, y = rs.randn(4, 64), rs.randn(4, 64)           # four samples: covariances of rank 3 in 64 dimensions
    (m1, S1), (m2, S2) = FRF.moments(x), FRF.moments(y)
    assert np.linalg.matrix_rank(S1) == 3
    for args in ((m1, S1, m2, S2), (m1, S1, m1, S1), (m1, S1, m2, _spd(rs, 64))):
        v = fr.frechet_distance(*args)
        assert np.isfinite(v) and v >= 0.0
    assert fr.frechet_distance(m1, S1, m1, S1) <= 1e-9


def test_agreement_with_scipy_sqrtm_on_random_spd_pairs():
    sl = pytest.importorskip("scipy.linalg")
    fr, rs = _fr(), np.random.RandomState(5)
    for d in (3, 16, 64):
        S1, S2, m1, m2 = _spd(rs, d), _spd(rs, d, 2.0), rs.randn(d), rs.randn(d)
        root = sl.sqrtm(S1.dot(S2))
        want = (m1 - m2).dot(m1 - m2) + np.trace(S1) + np.trace(S2) - 2.0 * np.trace(root).real
        assert abs(fr.frechet_distance(m1, S1, m2, S2) - want) <= 1e-8 * want, d


# ------------------------------------------------------------------------------------------------------------------ evaluate
def test_pooled_moments_from_per_class_sums_equal_two_pass_moments_of_the_concatenation():
    fr, rs = _fr(), np.random.RandomState(6)
    x = (rs.randn(500, 12) * rs.uniform(0.5, 2.0, 12) + rs.randn(12)).astype(np.float32)
    labels = rs.randint(5, size=500)
    mom = fr.moments_of(x, labels, 5)
    m, c = FRF.moments(x)
    assert mom.pooled[0] == 500 and mom.rejected == 0
    assert np.abs(mom.pooled[1] - m).max() <= 1e-12 * np.abs(m).max()
    assert np.abs(mom.pooled[2] - c).max() <= 1e-12 * np.abs(c).max()
    for k in range(5):
        mk, ck = FRF.moments(x[labels == k])
        assert mom.count[k] == (labels == k).sum()
        assert np.abs(mom.mean[k] - mk).max() <= 1e-12 * np.abs(mk).max() and np.abs(mom.cov[k] - ck).max() <= 1e-12 * np.abs(ck).max()


def test_a_class_with_one_sample_is_left_out_and_the_mean_is_over_the_rest():
    fr, rs = _fr(), np.random.RandomState(7)
    xa, xb = rs.randn(90, 8).astype(np.float32), (rs.randn(61, 8) + 0.5).astype(np.float32)
    la = np.arange(90) % 3
    lb = np.concatenate([np.arange(60) % 2, [2]])            # class 2 has one generated sample
    lb_bad = lb.copy()
    lb_bad[:2] = (-1, 3)                                       # two rows outside the classes
    r = fr.evaluate(fr.moments_of(xa, la, 3), fr.moments_of(xb, lb_bad, 3))
    assert r["left_out"] == [2] and r["classes_used"] == 2 and np.isnan(r["per_class"][2])
    assert (r["rejected_real"], r["rejected_generated"]) == (0, 2)
    want = [fr.frechet_distance(*FRF.moments(xa[la == k]), *FRF.moments(xb[lb_bad == k])) for k in (0, 1)]
    assert np.allclose(r["per_class"][:2], want, rtol=1e-9)
    assert abs(r["intra_class_frechet_distance"] - np.mean(want)) <= 1e-12 * np.mean(want)
    keep = (lb_bad >= 0) & (lb_bad < 3)
    pooled = fr.frechet_distance(*FRF.moments(xa), *FRF.moments(xb[keep]))
    assert abs(r["frechet_distance"] - pooled) <= 1e-9 * pooled
    # a stricter threshold leaves out more; with nothing left the mean is nan, not 0
    assert fr.evaluate(fr.moments_of(xa, la, 3), fr.moments_of(xb, lb, 3), min_count=31)["left_out"] == [0, 1, 2]
    assert np.isnan(fr.evaluate(fr.moments_of(xa, la, 3), fr.moments_of(xb, lb, 3), min_count=31)["intra_class_frechet_distance"])
    fr.json_ready(r)


def test_the_permutation_of_conditioning_labels_is_the_accuracy_metrics():
    fr = _fr()
    perm = np.roll(np.arange(10), 3)
    cm = np.full((10, 10), 0.01)
    cm[np.arange(10), perm] = 0.9
    labels = np.arange(30) % 10
    assert (fr.permuted_labels(labels, cm) == perm[labels]).all()


# --------------------------------------------------------------------------------------------------------------------- cache
def test_the_cache_is_reused_only_under_the_same_asset_count_and_calibration(tmp_path):
    fr, rs = _fr(), np.random.RandomState(8)
    path = os.path.join(str(tmp_path), fr.CACHE_NAME)
    calls = []

    def stub(seed):
        def compute():
            calls.append(seed)
            r = np.random.RandomState(seed)
            x = r.randn(40, 6).astype(np.float32)
            pairs = {"conv0": (r.randn(16).astype(np.float32), r.uniform(size=16).astype(np.float32)),
                     "fc": (r.randn(64).astype(np.float32), r.uniform(size=64).astype(np.float32))}
            return fr.moments_of(x, np.arange(40) % 4, 4), pairs
        return compute
    key = dict(asset_sha256="a" * 64, n_real=40, calibration_sha256=fr.array_sha256(rs.randn(3, 4)))
    m0, p0, reused = fr.real_statistics(path, key, stub(0))
    assert not reused and calls == [0] and os.path.exists(path)
    m1, p1, reused = fr.real_statistics(path, dict(key), stub(1))
    assert reused and calls == [0]
    assert all(np.array_equal(a, b) for a, b in zip(m0[:3], m1[:3])) and all(np.array_equal(a, b) for a, b in zip(m0.pooled, m1.pooled))
    assert sorted(p1) == ["conv0", "fc"] and all(np.array_equal(p0[k][i], p1[k][i]) for k in p0 for i in (0, 1))
    n = 1
    for change in (dict(asset_sha256="b" * 64), dict(n_real=41), dict(calibration_sha256=fr.array_sha256(rs.randn(3, 4)))):
        key = dict(key, **change)
        _, _, reused = fr.real_statistics(path, key, stub(n + 1))
        n += 1
        assert not reused and calls[-1] == n and len(calls) == n, change
        assert fr.real_statistics(path, key, stub(99))[2] and len(calls) == n          # the rewritten file serves the new key
    # a file that is not a cache at all is recomputed over, not an error
    open(path, "wb").write(b"not an archive")
    assert not fr.real_statistics(path, key, stub(50))[2] and fr.real_statistics(path, key, stub(51))[2]
    # hashes see dtype, shape and content
    a = np.arange(6, dtype=np.float32)
    assert len({fr.array_sha256(a), fr.array_sha256(a.reshape(2, 3)), fr.array_sha256(a.astype(np.float64)), fr.array_sha256(a + 1)}) == 4


def test_training_flags_default_to_off_and_bad_values_are_refused_before_anything_runs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    FLAGS = train_cifar.define_flags().parse([])
    assert (FLAGS.frechet_freq, FLAGS.frechet_samples, FLAGS.frechet_real_samples) == (0, 10000, 0)
    with pytest.raises(ValueError, match="frechet"):
        train_cifar.main(["--log_file", os.path.join(str(tmp_path), "log.txt"), "--frechet_freq", "2", "--frechet_samples", "50"])
    assert not os.path.exists(os.path.join(str(tmp_path), "log.txt"))
