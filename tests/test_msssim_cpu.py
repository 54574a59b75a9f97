"""Intra-class MS-SSIM without a GPU: the float64 restatement (tests/msssim_ref.py) against outputs of the reference's own functions
(tests/golden/ref_msssim.npz, recorded by tests/tools/record_msssim_golden.py), closed-form cases, the pair draw, the host arithmetic
of msssim.py, the training flags, and the argument checks of the entry point of csrc/msssim.hip (made before anything touches a
device)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import msssim_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("32x32x3", "28x28x1", "16x16x1", "17x23x3")
REL = 1e-10          # both sides float64; they differ by the reference's FFT rounding (measured: 1.4e-12 at most)


def _ms():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import msssim
    return msssim


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_msssim.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("tag", SHAPES)
def test_the_restatement_equals_the_reference_functions_on_the_recorded_inputs(golden, tag):
    ms = _ms()
    images, pairs, want, value = golden["images_" + tag], golden["pairs_" + tag], golden["scales_" + tag], float(golden["value_" + tag])
    assert images.dtype == np.uint8 and images.shape[1:] == tuple(int(v) for v in tag.split("x"))
    assert np.isfinite(want).all() and np.isfinite(value) and (want.min() < 0.5)          # (structured inputs; not a batch of ones)
    got = MR.scales(images, pairs)
    rel = np.abs(got - want) / np.abs(want)
    print("%s: per-scale values within %.2e relative, batch value %.12f against %.12f" % (tag, rel.max(), MR.combine(got), value))
    assert (rel <= REL).all()
    for combine in (MR.combine, ms.combine):
        assert abs(combine(got) - value) <= REL * value
    batch = MR.msssim(images[pairs[:, 0]], images[pairs[:, 1]])
    assert abs(batch - value) <= REL * value


def test_a_noise_batch_the_reference_cannot_score_is_nan_here_too(golden):
    ms = _ms()
    assert np.isnan(float(golden["noise_value"]))
    sc = MR.scales(golden["noise_images"], golden["noise_pairs"])
    assert np.isfinite(sc).all() and sc.mean(axis=0)[0, :4].min() <= 0           # a contrast-structure mean is not positive
    assert np.isnan(MR.combine(sc)) and np.isnan(ms.combine(sc))
    assert np.isnan(ms.combine(np.zeros((0, 2, 5))))                             # no pair at all


# ------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("shape", [(32, 32, 3), (28, 28, 1), (16, 16, 1), (17, 23, 3)])
def test_identical_constant_and_black_against_white_pairs(shape):
    ms = _ms()
    x = np.random.RandomState(3).randint(0, 256, size=shape)
    same = MR.pair_scales(x, x)
    assert np.abs(same - 1.0).max() <= 1e-12 and abs(ms.combine(same[None]) - 1.0) <= 1e-12
    for a, b in ((0, 0), (7, 7), (255, 255), (7, 200), (0, 255)):
        sc = MR.pair_scales(np.full(shape, a), np.full(shape, b))
        lum = (2.0 * a * b + MR.C1) / (a * a + b * b + MR.C1)                    # no variance: cs = c2 / c2, ssim = the luminance factor
        assert np.abs(sc[0] - 1.0).max() <= 1e-9 and np.abs(sc[1] - lum).max() <= 1e-9 * max(lum, 1e-3), (a, b)
        assert abs(ms.combine(sc[None]) - lum ** MR.WEIGHTS[4]) <= 1e-9
    assert abs(ms.combine(MR.pair_scales(np.zeros(shape), np.full(shape, 255))[None]) - (MR.C1 / (255.0 ** 2 + MR.C1)) ** 0.1333) <= 1e-9


def test_level_sizes_and_windows_of_the_smallest_shape():
    x = np.zeros((16, 16, 1))
    sizes = []
    for _ in range(5):
        sizes.append((x.shape[0], min(11, x.shape[0], x.shape[1])))
        x = MR._half(x)
    assert sizes == [(16, 11), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert MR._half(np.arange(15.0).reshape(5, 3, 1))[:, :, 0].tolist() == [[2.0, 3.5], [8.0, 9.5], [12.5, 14.0]]     # odd: last row / column repeated
    for s in (1, 2, 3, 8, 11):
        g = MR.taps(s)
        assert abs(g.sum() - 1.0) <= 1e-15 and np.allclose(g, g[::-1], rtol=0, atol=1e-16)


# ------------------------------------------------------------------------------------------------------------------ the pairs
def test_class_pairs_are_distinct_ordered_within_their_class_and_deterministic():
    ms = _ms()
    K = 6
    labels = np.array([0] * 40 + [1] * 5 + [2] * 1 + [4] * 2 + [5] * 30 + [-1, 6, 99])        # class 2: one row; class 3: none; 3 rejected
    labels = labels[np.random.RandomState(1).permutation(len(labels))]
    state = np.random.get_state()
    cp = ms.class_pairs(labels, K, 20, seed=11)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # the global stream did not move
    pairs, off = cp["pairs"], cp["off"]
    assert pairs.dtype == np.int32 and pairs.shape == (off[-1], 2) and len(off) == K + 2
    assert cp["rejected"] == 3 and cp["rows"].tolist() == [40, 5, 1, 0, 2, 30]
    assert (off[1:K + 1] - off[:K]).tolist() == [20, 10, 0, 0, 1, 20]            # small classes take all of their pairs
    for c in range(K):
        seg = pairs[off[c]:off[c + 1]]
        assert (labels[seg] == c).all() and (seg[:, 0] < seg[:, 1]).all()
        assert len({(int(i), int(j)) for i, j in seg}) == len(seg)
    assert sorted(map(tuple, pairs[off[1]:off[2]].tolist())) == sorted(
        (int(i), int(j)) for a, i in enumerate(np.flatnonzero(labels == 1)) for j in np.flatnonzero(labels == 1)[a + 1:])
    pooled = pairs[off[K]:off[K + 1]]
    ok = (labels >= 0) & (labels < K)
    assert len(pooled) == 20 and ok[pooled].all() and (pooled[:, 0] < pooled[:, 1]).all()
    assert len({(int(i), int(j)) for i, j in pooled}) == 20
    again = ms.class_pairs(labels, K, 20, seed=11)
    assert np.array_equal(again["pairs"], pairs) and np.array_equal(again["off"], off)
    other = ms.class_pairs(labels, K, 20, seed=12)
    assert not np.array_equal(other["pairs"], pairs)
    for bad in (dict(n_classes=0), dict(pairs=0)):
        with pytest.raises(ValueError, match="class_pairs"):
            ms.class_pairs(labels, **dict(dict(n_classes=K, pairs=20, seed=1), **bad))


def test_every_way_of_drawing_gives_distinct_values_in_range_and_unranking_is_the_pair_list():
    ms = _ms()
    i, j = ms._unrank(np.arange(10))
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (0, 4), (1, 4), (2, 4), (3, 4)]
    n = 50000                                                        # the pooled segment of a whole training set
    total = n * (n - 1) // 2
    i, j = ms._unrank(np.array([0, total - 1, total // 2, 2 ** 30]))
    assert (i < j).all() and (j < n).all() and (i[1], j[1]) == (n - 2, n - 1)
    assert (j * (j - 1) // 2 + i).tolist() == [0, total - 1, total // 2, 2 ** 30]
    for total, k in ((5, 9), (9, 9), (12, 9), (18, 9), (19, 9), (10 ** 9, 1000)):         # all; a permutation's head; rejection
        got = ms._draw(np.random.RandomState(0), total, k)
        assert len(got) == min(total, k) == len(set(got.tolist())) and got.min() >= 0 and got.max() < total


# ---------------------------------------------------------------------------------------------------------------- summarise
def _hand_made(ms):
    """Class 0: two pairs averaging 0.5 at every scale; class 1: a non-positive cs mean at scale 3 (undefined); class 2: one row (left
    out); class 3: all ones; pooled: 0.25 everywhere."""
    cp = dict(pairs=np.zeros((7, 2), np.int32), off=np.array([0, 2, 4, 4, 5, 7]), rows=np.array([3, 4, 1, 2]), rejected=2)
    sc = np.zeros((7, 2, 5))
    sc[0], sc[1] = 0.25, 0.75
    sc[2], sc[3] = 0.5, 0.5
    sc[2, 0, 3], sc[3, 0, 3] = -0.7, 0.7
    sc[4] = 1.0
    sc[5:] = 0.25
    return cp, sc


def test_summarise_counts_only_classes_defined_on_both_sides_and_json_ready_writes_null_for_nan():
    ms = _ms()
    cp, sc = _hand_made(ms)
    w = MR.WEIGHTS.sum()
    real = ms.summarise(sc, cp)
    assert np.allclose(real["per_class"][[0, 3]], [0.5 ** w, 1.0], rtol=1e-15) and np.isnan(real["per_class"][[1, 2]]).all()
    assert real["left_out"] == [2] and real["undefined"] == [1] and real["pairs_used"].tolist() == [2, 2, 0, 1]
    assert real["msssim"] == pytest.approx(0.25 ** w, rel=1e-15)
    assert real["intra_class_msssim"] == pytest.approx((0.5 ** w + 1.0) / 2, rel=1e-15)
    assert real["intra_class_msssim_se"] == pytest.approx(np.std([0.5 ** w, 1.0], ddof=1) / np.sqrt(2), rel=1e-15)
    assert real["classes_compared"] == 0 and real["classes_above_real"] == 0 and np.isnan(real["intra_class_msssim_real"])
    assert np.array_equal(real["per_class_scales"][0], np.full((2, 5), 0.5)) and np.isnan(real["per_class_scales"][2]).all()
    assert real["per_class_scales"][1][0, 3] == 0.0                   # (the scale means of an undefined class are still reported)
    # generated: class 0 higher than real, class 1 now defined (the real side is not), class 3 lower than real
    gen = sc.copy()
    gen[0], gen[1] = 0.75, 0.75
    gen[2, 0, 3] = 0.7
    gen[4] = 0.9
    got = ms.summarise(gen, cp, real)
    assert not np.isnan(got["per_class"][1]) and got["undefined"] == [] and got["left_out"] == [2]
    assert got["classes_compared"] == 2 and got["classes_above_real"] == 1                  # classes 0 and 3; only class 0 is above
    assert got["intra_class_msssim_real"] == real["intra_class_msssim"] and got["msssim_real"] == real["msssim"]
    assert np.array_equal(np.isnan(got["real_per_class"]), [False, True, True, False])
    got.update(rejected_real=2, rejected_generated=0)
    ready = ms.json_ready(got)
    assert ready["per_class"][2] is None and ready["real_per_class"][1] is None and ready["per_class_scales"][2][0][0] is None
    assert ready["classes_above_real"] == 1 and ready["pairs_used"] == [2, 2, 0, 1] and ready["left_out"] == [2]
    json.dumps(ready)
    json.dumps(ms.json_ready(dict(real, rejected_real=0, rejected_generated=0)))
    with pytest.raises(ValueError, match="summarise"):
        ms.summarise(sc[:-1], cp)
    # no class defined at all: nan, not zero
    none = ms.summarise(np.zeros((0, 2, 5)), dict(pairs=np.zeros((0, 2), np.int32), off=np.zeros(4, np.int64), rows=np.array([1, 0]), rejected=0))
    assert np.isnan(none["intra_class_msssim"]) and np.isnan(none["intra_class_msssim_se"]) and np.isnan(none["msssim"])
    assert none["left_out"] == [0, 1] and none["undefined"] == []


def test_images_are_taken_in_the_layouts_of_the_data_sets_and_refused_otherwise():
    ms = _ms()
    rows = np.arange(2 * 3072).reshape(2, 3072) % 256
    x = ms.as_uint8_nhwc(rows)
    assert x.dtype == np.uint8 and x.shape == (2, 32, 32, 3) and x[1, 4, 5, 2] == rows[1, 2 * 1024 + 4 * 32 + 5]
    assert ms.as_uint8_nhwc(np.zeros((3, 784))).shape == (3, 28, 28, 1) and ms.as_uint8_nhwc(np.zeros((3, 28, 28), np.int32)).shape == (3, 28, 28, 1)
    assert ms.as_uint8_nhwc(np.full((1, 17, 23, 3), 254.6)).max() == 255
    for bad in (np.zeros((2, 100)), np.zeros((2, 15, 16, 1)), np.zeros((2, 33, 32, 3)), np.zeros((2, 32, 32, 2)), np.full((1, 32, 32, 3), 256),
                np.full((1, 32, 32, 3), -1)):
        with pytest.raises(ValueError, match="msssim"):
            ms.as_uint8_nhwc(bad)


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_training_flags_default_to_off_and_bad_values_are_refused_before_anything_runs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    FLAGS = train_cifar.define_flags().parse([])
    assert (FLAGS.msssim_freq, FLAGS.msssim_samples, FLAGS.msssim_real_samples, FLAGS.msssim_pairs) == (0, 10000, 0, 1000)
    log = os.path.join(str(tmp_path), "log.txt")
    for bad in (["--msssim_freq", "2", "--msssim_samples", "50"], ["--msssim_freq", "-1"], ["--msssim_real_samples", "-1"],
                ["--msssim_freq", "2", "--msssim_pairs", "0"], ["--msssim_freq", "2", "--msssim_pairs", "-5"]):
        with pytest.raises(ValueError, match="msssim"):
            train_cifar.main(["--log_file", log] + bad)
        assert not os.path.exists(log)


def test_the_evaluator_checks_its_arguments_before_it_builds_a_context():
    ms = _ms()
    for kw in (dict(n_classes=0), dict(pairs=0), dict(pairs=-1)):
        with pytest.raises(ValueError, match="MsssimEvaluator"):
            ms.MsssimEvaluator(**dict(dict(n_classes=10, pairs=1000), **kw))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_entry_point_and_check_arguments_without_a_device():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    assert re.search(r"\brcgan_msssim_pairs\s*\(", hdr) and "rcgan_msssim_pairs" in _lib.SIGNATURES
    x = (C.c_uint8 * (4 * 32 * 32 * 3))()
    pairs = (C.c_int32 * 8)(0, 1, 2, 3)
    out = (C.c_float * 40)()
    p = lambda a: C.cast(a, C.c_void_p) if a is not None else None
    for lib in (_lib.load(), _lib.load("f16")):
        call = lambda n=4, h=32, w=32, c=3, n_pairs=2, xx=x, pp=pairs, oo=out: lib.rcgan_msssim_pairs(None, n, h, w, c, n_pairs, p(xx), p(pp), p(oo))
        for bad in (dict(n=0), dict(n=-2), dict(n_pairs=0), dict(n_pairs=-1), dict(c=0), dict(c=2), dict(c=4), dict(h=15), dict(w=15), dict(h=33),
                    dict(w=33), dict(h=0), dict(w=-32), dict(xx=None), dict(pp=None), dict(oo=None)):
            assert call(**bad) == _lib.EINVALID_ARG, bad
        assert call() == _lib.EINVALID_ARG                           # legal arguments, but no context
        assert all(v == 0.0 for v in out)                            # nothing was written
