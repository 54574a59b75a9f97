"""Intra-class MS-SSIM on the GPU: MsssimEvaluator on template images against the float64 restatement (tests/msssim_ref.py) fed the
same pairs; the orderings the number exists for (a collapsed set is MORE alike than the real one in every class, a set whose labels
are shuffled across classes LESS); what is left out; the stand-alone tool; the training command line.

Agreement: every per-scale mean of a pair is within TOL = 1e-4 of the restatement (the kernel's derived bound, csrc/msssim.hip), so
is a mean over pairs, and the value prod m_l^{w_l} lies between the products taken at m_l - TOL and m_l + TOL."""
import json
import os
import re

import numpy as np
import pytest

from tests import msssim_ref as MR
from tests.train_launch import launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K, PER_CLASS, PAIRS, TOL = 4, 24, 50, 1e-4


def _templates(seed, labels):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as DT
    return DT.template_images(np.random.RandomState(seed), np.asarray(labels)).astype(np.uint8)            # [n,3072] CHW rows


def _nhwc(rows):
    return rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)


def _reference(ms, rows, labels, seed):
    """-> (per-class values, pooled value, per-class [K,2,5] scale means) of the restatement on the evaluator's own pairs."""
    cp = ms.class_pairs(labels, K, PAIRS, seed)
    sc = MR.scales(_nhwc(rows), cp["pairs"])
    off = cp["off"]
    per = np.array([MR.combine(sc[off[c]:off[c + 1]]) for c in range(K)])
    means = np.stack([sc[off[c]:off[c + 1]].mean(axis=0) if off[c + 1] > off[c] else np.full((2, 5), np.nan) for c in range(K)])
    return per, MR.combine(sc[off[K]:off[K + 1]]), means, sc[off[K]:off[K + 1]].mean(axis=0)


def _between(got, means):
    """got lies between the products of the scale means moved down and up by TOL."""
    base = np.concatenate([means[0, :4], means[1, 4:]])
    assert (base - TOL > 0).all()
    return np.prod((base - TOL) ** MR.WEIGHTS) <= got <= np.prod((base + TOL) ** MR.WEIGHTS)


@pytest.fixture(scope="module")
def world():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import msssim as ms
    labels = np.random.RandomState(5).permutation(np.repeat(np.arange(K), PER_CLASS))
    real, gen = _templates(31, labels), _templates(32, labels)
    ev = ms.MsssimEvaluator(K, pairs=PAIRS)
    ev.prepare_real(real, labels)
    w = dict(ms=ms, ev=ev, labels=labels, real=real, gen=gen, got=ev.evaluate(_nhwc(gen), labels),          # (both layouts are taken)
             ref_real=_reference(ms, real, labels, ev.seed), ref_gen=_reference(ms, gen, labels, ev.seed))
    yield w
    ev.close()


def test_the_evaluator_agrees_with_the_float64_restatement_on_the_same_pairs(world):
    got, (per, pooled, means, pooled_means), (rper, rpooled, rmeans, rpooled_means) = world["got"], world["ref_gen"], world["ref_real"]
    print("intra-class MS-SSIM %.5f +- %.5f (real %.5f), pooled %.5f (real %.5f); per class %s against the restatement's %s"
          % (got["intra_class_msssim"], got["intra_class_msssim_se"], got["intra_class_msssim_real"], got["msssim"], got["msssim_real"],
             np.array2string(got["per_class"], precision=5), np.array2string(per, precision=5)))
    assert got["pairs_used"].tolist() == [PAIRS] * K and got["left_out"] == [] and got["undefined"] == []
    assert (got["rejected_real"], got["rejected_generated"]) == (0, 0)
    assert np.abs(got["per_class_scales"] - means).max() <= TOL
    for c in range(K):
        assert _between(got["per_class"][c], means[c]) and _between(got["real_per_class"][c], rmeans[c]), c
    assert _between(got["msssim"], pooled_means) and _between(got["msssim_real"], rpooled_means)
    assert got["intra_class_msssim"] == pytest.approx(got["per_class"].mean(), rel=1e-15)
    assert got["intra_class_msssim_se"] == pytest.approx(got["per_class"].std(ddof=1) / 2.0, rel=1e-12)
    assert got["intra_class_msssim_real"] == pytest.approx(got["real_per_class"].mean(), rel=1e-15)
    assert got["classes_compared"] == K and got["classes_above_real"] == int((got["per_class"] > got["real_per_class"]).sum())
    assert got["msssim"] < got["intra_class_msssim"]                 # pairs regardless of class are less alike than pairs of one class
    again = world["ev"].evaluate(world["gen"], world["labels"])
    assert again["per_class"].tobytes() == got["per_class"].tobytes() and again["msssim"] == got["msssim"]      # same pairs, same bits


def test_a_collapsed_set_scores_above_the_real_set_in_every_class_and_shuffled_labels_below(world):
    ev, labels, got = world["ev"], world["labels"], world["got"]
    rs = np.random.RandomState(6)
    one = _templates(33, np.arange(K))                               # one image per class ...
    collapsed = np.clip(one[labels].astype(np.float64) + 2.0 * rs.randn(len(labels), 3072), 0, 255)        # ... plus small noise
    r = ev.evaluate(collapsed, labels)
    print("collapsed: per class %s against real %s" % (np.array2string(r["per_class"], precision=4), np.array2string(r["real_per_class"], precision=4)))
    assert (r["per_class"] > r["real_per_class"]).all() and r["classes_above_real"] == K and r["classes_compared"] == K
    assert r["intra_class_msssim"] > 0.9 > got["intra_class_msssim"]
    shuffled = rs.permutation(labels)                                # every class is now a mixture of all classes
    r = ev.evaluate(world["gen"], shuffled)
    print("labels shuffled: intra-class %.5f against real %.5f (clean labels: %.5f)" % (r["intra_class_msssim"], r["intra_class_msssim_real"], got["intra_class_msssim"]))
    assert r["intra_class_msssim"] < r["intra_class_msssim_real"] and r["intra_class_msssim"] < got["intra_class_msssim"]


def test_a_class_with_one_row_is_left_out_and_rows_with_a_foreign_label_are_counted(world):
    ev, labels = world["ev"], world["labels"].copy()
    rows3 = np.flatnonzero(labels == 3)
    labels[rows3[1:]] = K + 2                                        # class 3 keeps one row; 23 rows carry a label outside [0, K)
    r = ev.evaluate(world["gen"], labels)
    assert r["left_out"] == [3] and r["undefined"] == [] and np.isnan(r["per_class"][3]) and r["pairs_used"].tolist() == [PAIRS] * 3 + [0]
    assert r["rejected_generated"] == PER_CLASS - 1 and r["classes_compared"] == K - 1
    assert not np.isnan(r["per_class"][:3]).any() and r["intra_class_msssim"] == pytest.approx(r["per_class"][:3].mean(), rel=1e-15)
    json.dumps(world["ms"].json_ready(r))


def test_the_stand_alone_tool_prints_the_evaluators_numbers_as_one_json_line(world, tmp_path, capsys):
    ms = world["ms"]
    a, b = os.path.join(str(tmp_path), "real.npz"), os.path.join(str(tmp_path), "generated.npz")
    np.savez(a, images=world["real"], labels=world["labels"])
    np.savez(b, images=_nhwc(world["gen"]), labels=world["labels"])
    ms.main(["--real", a, "--generated", b, "--pairs", str(PAIRS)])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    assert r["per_class"] == [float(v) for v in world["got"]["per_class"]] and r["msssim"] == world["got"]["msssim"]
    assert r["classes_compared"] == K and r["pairs_used"] == [PAIRS] * K


# ------------------------------------------------------------------------------------------------------------- command line
def test_training_logs_the_lines_at_every_period_and_at_the_end(tmp_path):
    text, _ = launch(tmp_path, ["--msssim_freq", "2", "--msssim_samples", "200", "--msssim_real_samples", "400", "--msssim_pairs", "20"], "m1")
    num = r"(-?[\d.]+(?:e[-+]?\d+)?|nan)"
    pooled = re.findall(r"INFO\s+msssim: %s$" % num, text, flags=re.M)
    intra = re.findall(r"INFO\s+intra_class_msssim: %s \+- %s \((\d+) of 10 classes\), real %s$" % (num, num, num), text, flags=re.M)
    above = re.findall(r"INFO\s+msssim_classes_above_real: (\d+) of (\d+)$", text, flags=re.M)
    assert len(pooled) == len(intra) == len(above) == 3, text[-3000:]              # iterations 2 and 4, and the end of training
    assert all(0.0 < float(a[3]) < 1.0 for a in intra)                            # the real set's value: template classes, always defined
    assert all(int(a) <= int(b) <= 10 for a, b in above)
    assert len(re.findall(r"msssim real set: 400 images, 20 pairs per class", text)) == 1
