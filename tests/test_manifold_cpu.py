"""k-NN precision / recall / density / coverage without a GPU: the host arithmetic of manifold.py against a hand-worked example and
against the brute-force float64 restatement (tests/manifold_ref.py), what is left out and what is rejected, the two entry points of
csrc/knn.hip in both libraries and their argument checks (made before anything touches a device), and the training flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import manifold_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mf():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import manifold
    return manifold


def _host_vectors(real, gen, k):
    """(count_g, count_r, nearest2_r, radius2_r) of one segment from the restatement's primitives."""
    rad_r, rad_g = MR.radii(real, k), MR.radii(gen, k)
    count_g, _ = MR.counts_nearest(gen, real, rad_r)
    count_r, nearest_r = MR.counts_nearest(real, gen, rad_g)
    return count_g, count_r, nearest_r, rad_r


def _host_evaluate(mf, real, rl, gen, gl, K, k):
    """manifold.summarise fed by the restatement's primitives in the layouts the evaluator uses (pooled: accepted rows in original
    order; grouped: a stable sort by class)."""
    rok, gok = (rl >= 0) & (rl < K), (gl >= 0) & (gl < K)
    real, rl, gen, gl = real[rok], rl[rok], gen[gok], gl[gok]
    ro, go = np.argsort(rl, kind="stable"), np.argsort(gl, kind="stable")
    off_r = np.concatenate([[0], np.cumsum(np.bincount(rl, minlength=K))])
    off_g = np.concatenate([[0], np.cumsum(np.bincount(gl, minlength=K))])
    R, G = real[ro], gen[go]
    rad_r, _ = MR.radii_segmented(R, off_r, k)
    rad_g, _ = MR.radii_segmented(G, off_g, k)
    count_g, _, _ = MR.ball_segmented(G, off_g, R, off_r, rad_r)
    count_r, nearest_r, _ = MR.ball_segmented(R, off_r, G, off_g, rad_g)
    out = mf.summarise(count_g, count_r, nearest_r, rad_r, off_g, off_r, k, _host_vectors(real, gen, k))
    out.update(rejected_real=int((~rok).sum()), rejected_generated=int((~gok).sum()))
    return out


def _same(a, b):
    for m in MR.METRICS:
        for key in (m, "intra_class_" + m):
            assert (np.isnan(a[key]) and np.isnan(b[key])) or a[key] == b[key], (key, a[key], b[key])
        assert np.array_equal(a["per_class"][m], b["per_class"][m], equal_nan=True), m
    assert a["left_out"] == b["left_out"] and a["classes_used"] == b["classes_used"]
    assert (a["rejected_real"], a["rejected_generated"]) == (b["rejected_real"], b["rejected_generated"])


# --------------------------------------------------------------------------------------------------------- the four numbers
def test_a_hand_worked_example_on_a_line():
    """k = 1, one dimension.  Real rows r = (0, 1, 3, -20), generated rows g = (0.5, 4, 10).

    Radii (distance to the nearest OTHER row of the same set), squared:
      real: 0 -> 1 (to 1); 1 -> 1 (to 0); 3 -> 4 (to 1); -20 -> 400 (to 0)           generated: 0.5 -> 12.25; 4 -> 12.25; 10 -> 36
    Real balls around each g:    0.5 is within 1 of 0 and of 1 (0.25 <= 1), not within 2 of 3 (6.25 > 4), not of -20 -> 2
                                 4 is within 2 of 3 (1 <= 4) only -> 1;    10 is in no ball (49 > 4, 81, 100 > 1, 900 > 400) -> 0
      precision = 2/3 (two of three g are in some real ball), density = (2 + 1 + 0) / (1 * 3) = 1
    Generated balls around each r (3.5, 3.5 and 6 wide):  0 -> {0.5} = 1;  1 -> {0.5, 4} = 2;  3 -> {0.5, 4} = 2 (49 > 36);  -20 -> 0
      recall = 3/4
    Nearest g of each r against r's own radius:  0: 0.25 <= 1;  1: 0.25 <= 1;  3: 1 <= 4;  -20: 420.25 > 400
      coverage = 3/4"""
    mf = _mf()
    real, gen = np.array([[0.0], [1.0], [3.0], [-20.0]]), np.array([[0.5], [4.0], [10.0]])
    count_g, count_r, nearest_r, rad_r = _host_vectors(real, gen, 1)
    assert rad_r.tolist() == [1.0, 1.0, 4.0, 400.0] and MR.radii(gen, 1).tolist() == [12.25, 12.25, 36.0]
    assert count_g.tolist() == [2, 1, 0] and count_r.tolist() == [1, 2, 2, 0] and nearest_r.tolist() == [0.25, 0.25, 1.0, 420.25]
    want = dict(precision=2.0 / 3.0, recall=0.75, density=1.0, coverage=0.75)
    assert mf.metrics(count_g, count_r, nearest_r, rad_r, 1) == want
    assert MR.metrics_of(real, gen, 1) == want


def test_two_identical_sets():
    mf, rs = _mf(), np.random.default_rng(0)
    x = rs.standard_normal((80, 5)).astype(np.float32)
    for k in (1, 3, 5):
        got, ref = mf.metrics(*_host_vectors(x, x, k), k), MR.metrics_of(x, x, k)
        assert got == ref
        assert got["precision"] == got["recall"] == got["coverage"] == 1.0
        # every row lies in its own ball and in those of the k rows it is a neighbour of on average
        assert got["density"] >= (k + 1.0) / k


def test_one_real_point_repeated_has_full_precision_and_covers_almost_nothing():
    mf, rs = _mf(), np.random.default_rng(1)
    k = 3
    real = rs.standard_normal((60, 4)).astype(np.float32)
    gen = np.repeat(real[7:8], 20, axis=0)
    got, ref = mf.metrics(*_host_vectors(real, gen, k), k), MR.metrics_of(real, gen, k)
    assert got == ref
    assert got["precision"] == 1.0                      # the point is in its own ball
    assert got["recall"] == 1.0 / 60                    # zero radii: only the repeated row itself is inside a generated ball
    # covered: exactly the real rows whose own ball reaches the repeated row -- that row itself and the few it is a near neighbour of
    reach = int((MR.dist2(real, real[7:8])[:, 0] <= MR.radii(real, k)).sum())
    assert got["coverage"] == reach / 60.0 and 1 <= reach < 30


def test_small_classes_are_left_out_and_rejected_rows_are_counted():
    mf, rs = _mf(), np.random.default_rng(2)
    K, k = 5, 3
    real, gen = rs.standard_normal((90, 6)).astype(np.float32), (1.1 * rs.standard_normal((70, 6)) + 0.2).astype(np.float32)
    rl, gl = np.arange(90) % 4, np.arange(70) % 5              # class 4 has no real row
    gl[gl == 2] = np.where(np.arange((gl == 2).sum()) < k, 2, 0)    # class 2: exactly k generated rows
    rl[:3], gl[:2] = (-1, 5, 99), (-7, 5)
    got, ref = _host_evaluate(mf, real, rl, gen, gl, K, k), MR.evaluate(real, rl, gen, gl, K, k)
    _same(got, ref)
    assert got["left_out"] == [2, 4] and got["classes_used"] == 3
    assert (got["rejected_real"], got["rejected_generated"]) == (3, 2)
    for m in MR.METRICS:
        assert np.isnan(got["per_class"][m][[2, 4]]).all() and not np.isnan(got["per_class"][m][[0, 1, 3]]).any()
        assert got["intra_class_" + m] == pytest.approx(np.mean(got["per_class"][m][[0, 1, 3]]), rel=1e-15)
    ready = mf.json_ready(got)
    assert ready["per_class"]["recall"][2] is None and ready["left_out"] == [2, 4]
    import json
    json.dumps(ready)
    # nothing left: nan, not 0
    none = _host_evaluate(mf, real[:8], np.arange(8) % 4, gen[:8], np.arange(8) % 4, 4, k)
    assert none["classes_used"] == 0 and all(np.isnan(none["intra_class_" + m]) for m in MR.METRICS)
    assert not np.isnan(none["precision"])                         # the pooled sets (8 rows each) are large enough


def test_metrics_refuses_mismatched_vectors_and_an_empty_side_is_nan():
    mf = _mf()
    with pytest.raises(ValueError):
        mf.metrics([1, 2], [1, 2, 3], [0.0, 0.0], [1.0, 1.0, 1.0], 1)
    with pytest.raises(ValueError):
        mf.metrics([1], [1], [0.0], [1.0], 0)
    assert all(np.isnan(v) for v in mf.metrics([], [1], [0.0], [1.0], 1).values())


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_entry_points_and_check_arguments_without_a_device():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in ("rcgan_knn_radius", "rcgan_ball_query"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    x = (C.c_float * 1024)()
    off = (C.c_int32 * 8)(0, 4)
    out = (C.c_float * 16)()
    cnt = (C.c_int32 * 16)()
    p = lambda a: C.cast(a, C.c_void_p) if a is not None else None
    for lib in (_lib.load(), _lib.load("f16")):
        radius = lambda n, d, k, s, xx=x, oo=off, rr=out: lib.rcgan_knn_radius(None, n, d, k, s, p(xx), p(oo), p(rr))
        for bad in ((0, 4, 1, 1), (-1, 4, 1, 1), (4, 0, 1, 1), (4, 257, 1, 1), (4, 4, 0, 1), (4, 4, 17, 1), (4, 4, 1, 0), (4, 4, 1, 1025)):
            assert radius(*bad) == _lib.EINVALID_ARG, bad
        for missing in (dict(xx=None), dict(oo=None), dict(rr=None)):
            assert radius(4, 4, 1, 1, **missing) == _lib.EINVALID_ARG, missing
        assert radius(4, 4, 1, 1) == _lib.EINVALID_ARG               # legal arguments, but no context
        ball = lambda nq, nr, d, s, q=x, qo=off, r=x, ro=off, rad=out, c=cnt, nn=out: \
            lib.rcgan_ball_query(None, nq, nr, d, s, p(q), p(qo), p(r), p(ro), p(rad), p(c), p(nn))
        for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 257, 1), (4, 4, 4, 0), (4, 4, 4, 1025), (-3, 4, 4, 1)):
            assert ball(*bad) == _lib.EINVALID_ARG, bad
        for missing in (dict(q=None), dict(qo=None), dict(r=None), dict(ro=None), dict(rad=None)):
            assert ball(4, 4, 4, 1, **missing) == _lib.EINVALID_ARG, missing
        assert ball(4, 4, 4, 1) == _lib.EINVALID_ARG
        assert all(v == 0.0 for v in out) and all(v == 0 for v in cnt)          # nothing was written


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_training_flags_default_to_off_and_bad_values_are_refused_before_anything_runs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    FLAGS = train_cifar.define_flags().parse([])
    assert (FLAGS.prdc_freq, FLAGS.prdc_samples, FLAGS.prdc_real_samples, FLAGS.prdc_k) == (0, 10000, 0, 5)
    log = os.path.join(str(tmp_path), "log.txt")
    for bad in (["--prdc_freq", "2", "--prdc_samples", "50"], ["--prdc_freq", "-1"], ["--prdc_real_samples", "-1"],
                ["--prdc_freq", "2", "--prdc_k", "0"], ["--prdc_freq", "2", "--prdc_k", "17"]):
        with pytest.raises(ValueError, match="prdc"):
            train_cifar.main(["--log_file", log] + bad)
        assert not os.path.exists(log)


def test_the_evaluator_checks_k_and_the_class_count_before_it_builds_a_classifier():
    mf = _mf()
    for kw in (dict(k=0), dict(k=17), dict(n_classes=0), dict(n_classes=1025)):
        with pytest.raises(ValueError, match="ManifoldEvaluator"):
            mf.ManifoldEvaluator(**dict(dict(n_classes=10, k=5), **kw))
