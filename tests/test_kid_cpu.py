"""Kernel distance without a GPU: the host arithmetic of kid.py against the brute-force float64 restatement (tests/kid_ref.py), what
is left out (nan, not 0), unbiasedness measured against the plug-in estimate, the entry point of csrc/ksum.hip in both libraries and
its argument checks (made before anything touches a device), and the training flags."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import kid_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


def _kid():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import kid
    return kid


def _features(seed, n, d):
    return np.abs(np.random.RandomState(seed).randn(n, d)).astype(np.float32)


def _host_evaluate(kid, real, rl, gen, gl, K, subset_size):
    """kid.summarise fed by the restatement's row sums in the layouts the evaluator uses (pooled: accepted rows in original order as
    one segment; grouped: a stable sort by class; blocks: the pooled rows under a block offset array)."""
    rok, gok = (rl >= 0) & (rl < K), (gl >= 0) & (gl < K)
    real, rl, gen, gl = real[rok], rl[rok], gen[gok], gl[gok]
    ro, go = np.argsort(rl, kind="stable"), np.argsort(gl, kind="stable")
    off_r = np.concatenate([[0], np.cumsum(np.bincount(rl, minlength=K))])
    off_g = np.concatenate([[0], np.cumsum(np.bincount(gl, minlength=K))])
    R, G = real[ro], gen[go]
    gamma, coef0 = kid.gamma_of(real.shape[1]), kid.COEF0
    sums = lambda q, qo, r, ro_, ex: KR.rowsum_segmented(q, qo, r, ro_, gamma, coef0, ex)[0]
    one_g, one_r = [0, len(gen)], [0, len(real)]
    boff = kid.block_offsets(len(gen), len(real), subset_size)
    blocks = (sums(gen, boff, gen, boff, True), sums(real, boff, real, boff, True), sums(gen, boff, real, boff, False), boff) if len(boff) > 1 else None
    out = kid.summarise(sums(G, off_g, G, off_g, True), sums(R, off_r, R, off_r, True), sums(G, off_g, R, off_r, False), off_g, off_r,
                        (sums(gen, one_g, gen, one_g, True), sums(real, one_r, real, one_r, True), sums(gen, one_g, real, one_r, False)), blocks)
    out.update(rejected_real=int((~rok).sum()), rejected_generated=int((~gok).sum()))
    return out


def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= REL * max(abs(a), abs(b))


def _same(got, ref):
    for key in ("kernel_distance", "intra_class_kernel_distance", "intra_class_kernel_distance_se", "subset_mean", "subset_std"):
        assert _close(got[key], ref[key]), (key, got[key], ref[key])
    assert np.array_equal(np.isnan(got["per_class"]), np.isnan(ref["per_class"]))
    for c, (a, b) in enumerate(zip(got["per_class"], ref["per_class"])):
        assert _close(a, b), (c, a, b)
    for key in ("subsets", "left_out", "classes_used", "rejected_real", "rejected_generated"):
        assert got[key] == ref[key], key


# ------------------------------------------------------------------------------------------------------------ the estimate
def test_unbiased_mmd2_equals_the_definition():
    kid = _kid()
    for seed, m, n, d in ((0, 24, 40, 64), (1, 2, 2, 3), (2, 130, 7, 67)):
        g, r = _features(seed, m, d), _features(seed + 100, n, d) + 0.1
        Kgg, Krr, Kgr = KR.kernel(g, g), KR.kernel(r, r), KR.kernel(g, r)
        got = kid.unbiased_mmd2(Kgg.sum() - np.trace(Kgg), Krr.sum() - np.trace(Krr), Kgr.sum(), m, n)
        want = KR.mmd2_unbiased(g, r)
        assert abs(got - want) <= REL * abs(want), (got, want)
    assert kid.gamma_of(64) == KR.gamma_of(64) == 1.0 / 64 and kid.COEF0 == 1.0
    for m, n in ((1, 5), (5, 1), (0, 9), (1, 1)):
        assert np.isnan(kid.unbiased_mmd2(0.0, 0.0, 3.0, m, n))


def test_summarise_equals_the_reference_with_classes_left_out_and_rows_rejected():
    kid = _kid()
    K, s = 5, 16
    real, gen = _features(3, 90, 8), _features(4, 70, 8) * 1.1
    rl, gl = np.arange(90) % 4, np.arange(70) % 5              # class 4 has no real row
    gl[gl == 2] = np.where(np.arange((gl == 2).sum()) < 1, 2, 0)    # class 2: exactly one generated row
    rl[:3], gl[:2] = (-1, 5, 99), (-7, 5)
    got, ref = _host_evaluate(kid, real, rl, gen, gl, K, s), KR.evaluate(real, rl, gen, gl, K, s)
    _same(got, ref)
    assert got["left_out"] == [2, 4] and got["classes_used"] == 3 and got["subsets"] == 4
    assert (got["rejected_real"], got["rejected_generated"]) == (3, 2)
    assert np.isnan(got["per_class"][[2, 4]]).all() and not np.isnan(got["per_class"][[0, 1, 3]]).any()
    assert got["intra_class_kernel_distance"] == pytest.approx(np.mean(got["per_class"][[0, 1, 3]]), rel=1e-15)
    assert got["intra_class_kernel_distance_se"] == pytest.approx(np.std(got["per_class"][[0, 1, 3]], ddof=1) / np.sqrt(3), rel=1e-15)
    ready = kid.json_ready(got)
    assert ready["per_class"][2] is None and ready["left_out"] == [2, 4]
    json.dumps(ready)


def test_no_class_left_and_no_subset_give_nan_not_zero():
    kid = _kid()
    real, gen = _features(5, 4, 6), _features(6, 4, 6)
    labels = np.arange(4)                                            # one row per class on either side
    got, ref = _host_evaluate(kid, real, labels, gen, labels, 4, 1000), KR.evaluate(real, labels, gen, labels, 4, 1000)
    _same(got, ref)
    assert got["classes_used"] == 0 and got["left_out"] == [0, 1, 2, 3]
    assert np.isnan(got["intra_class_kernel_distance"]) and np.isnan(got["intra_class_kernel_distance_se"])
    assert got["subsets"] == 0 and np.isnan(got["subset_mean"]) and np.isnan(got["subset_std"])
    assert not np.isnan(got["kernel_distance"])                      # the pooled sets (4 rows each) are large enough
    ready = kid.json_ready(got)
    assert ready["intra_class_kernel_distance"] is None and ready["subset_mean"] is None and ready["subsets"] == 0
    json.dumps(ready)
    # one class takes part: a mean, no standard error
    two = _host_evaluate(kid, real, labels // 2 * 3, gen, labels // 2 * 3, 4, 2)          # classes 0 and 3, two rows each
    assert two["classes_used"] == 2 and not np.isnan(two["intra_class_kernel_distance_se"])
    one = _host_evaluate(kid, real, np.zeros(4, int), gen, np.array([0, 0, 1, 2]), 4, 2)
    _same(one, KR.evaluate(real, np.zeros(4, int), gen, np.array([0, 0, 1, 2]), 4, 2))
    assert one["classes_used"] == 1 and not np.isnan(one["intra_class_kernel_distance"]) and np.isnan(one["intra_class_kernel_distance_se"])
    assert one["subsets"] == 2 and one["subset_std"] >= 0.0


def test_the_estimate_is_unbiased_where_the_plug_in_estimate_is_not():
    """Two samples of ONE distribution (fp32 |N(0,1)|, d = 64, 24 against 40 rows), 400 trials: the module's estimate averages zero
    within 3 standard errors; the plug-in estimate, written out here, sits at least 10 of its standard errors above zero -- so this
    test can tell the two apart."""
    kid = _kid()
    rs = np.random.RandomState(7)
    d, m, n, trials = 64, 24, 40, 400
    unbiased, plug_in = np.zeros(trials), np.zeros(trials)
    for t in range(trials):
        g, r = np.abs(rs.randn(m, d)).astype(np.float32), np.abs(rs.randn(n, d)).astype(np.float32)
        Kgg, Krr, Kgr = KR.kernel(g, g), KR.kernel(r, r), KR.kernel(g, r)
        unbiased[t] = kid.unbiased_mmd2(Kgg.sum() - np.trace(Kgg), Krr.sum() - np.trace(Krr), Kgr.sum(), m, n)
        plug_in[t] = Kgg.sum() / (m * m) + Krr.sum() / (n * n) - 2.0 * Kgr.sum() / (m * n)
    se = lambda v: v.std(ddof=1) / np.sqrt(trials)
    print("unbiased %.3e +- %.3e, plug-in %.3e +- %.3e" % (unbiased.mean(), se(unbiased), plug_in.mean(), se(plug_in)))
    assert abs(unbiased.mean()) <= 3.0 * se(unbiased)
    assert plug_in.mean() >= 10.0 * se(plug_in)


def test_block_offsets_cut_contiguous_subsets_of_the_smaller_side():
    kid = _kid()
    assert kid.block_offsets(70, 90, 16).tolist() == [0, 16, 32, 48, 64]
    assert kid.block_offsets(90, 31, 16).tolist() == [0, 16]
    assert kid.block_offsets(15, 90, 16).tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_entry_point_and_check_arguments_without_a_device():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    assert re.search(r"\brcgan_poly3_rowsum\s*\(", hdr) and "rcgan_poly3_rowsum" in _lib.SIGNATURES
    x = (C.c_float * 1024)()
    off = (C.c_int32 * 8)(0, 4)
    out = (C.c_double * 16)()
    p = lambda a: C.cast(a, C.c_void_p) if a is not None else None
    for lib in (_lib.load(), _lib.load("f16")):
        call = lambda nq, nr, d, s, gamma=0.25, coef0=1.0, q=x, qo=off, r=x, ro=off, o=out: \
            lib.rcgan_poly3_rowsum(None, nq, nr, d, s, p(q), p(qo), p(r), p(ro), gamma, coef0, 0, p(o))
        for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (-3, 4, 4, 1), (4, -1, 4, 1), (4, 4, 0, 1), (4, 4, 257, 1), (4, 4, 4, 0), (4, 4, 4, 1025)):
            assert call(*bad) == _lib.EINVALID_ARG, bad
        for bad in (dict(gamma=float("nan")), dict(gamma=float("inf")), dict(coef0=float("nan")), dict(coef0=-float("inf"))):
            assert call(4, 4, 4, 1, **bad) == _lib.EINVALID_ARG, bad
        for missing in (dict(q=None), dict(qo=None), dict(r=None), dict(ro=None), dict(o=None)):
            assert call(4, 4, 4, 1, **missing) == _lib.EINVALID_ARG, missing
        assert call(4, 4, 4, 1) == _lib.EINVALID_ARG                 # legal arguments, but no context
        assert all(v == 0.0 for v in out)                            # nothing was written


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_training_flags_default_to_off_and_bad_values_are_refused_before_anything_runs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    FLAGS = train_cifar.define_flags().parse([])
    assert (FLAGS.kid_freq, FLAGS.kid_samples, FLAGS.kid_real_samples, FLAGS.kid_subset_size) == (0, 10000, 0, 1000)
    log = os.path.join(str(tmp_path), "log.txt")
    for bad in (["--kid_freq", "2", "--kid_samples", "50"], ["--kid_freq", "-1"], ["--kid_real_samples", "-1"],
                ["--kid_freq", "2", "--kid_subset_size", "1"], ["--kid_freq", "2", "--kid_subset_size", "0"]):
        with pytest.raises(ValueError, match="kid"):
            train_cifar.main(["--log_file", log] + bad)
        assert not os.path.exists(log)


def test_the_evaluator_checks_the_class_count_and_the_subset_size_before_it_builds_a_classifier():
    kid = _kid()
    for kw in (dict(n_classes=0), dict(n_classes=1025), dict(subset_size=1), dict(subset_size=0)):
        with pytest.raises(ValueError, match="KernelDistanceEvaluator"):
            kid.KernelDistanceEvaluator(**dict(dict(n_classes=10, subset_size=1000), **kw))
