"""Nearest-training-image metrics on the GPU: NeighbourEvaluator against the brute-force restatement (tests/neighbours_ref.py), what
the numbers separate, what is left out, the stand-alone tool and the training command line.

T = 3000 template images (seed 1234), H = 600 of seed 1235, and as generated sets: a fresh draw of 600 (seed 1236); 600 training images
drawn at random + N(0, 2^2) noise, clipped; half fresh, half copies; one image per class + N(0, 2^2) (collapsed).  The restatement
alone gives (checked on the CPU): fresh copy rate 0.25 against 0.25 held out, z -0.72, 1-NN accuracy 0.50; copies copy rate 1.00,
z -29.99; half 0.64, z -14.9; collapsed generated-side accuracy 1.00.

The kernel is exact, so the evaluator must EQUAL the restatement: distances, indices and counts identical, every ratio of counts to
1e-12 and z to 1e-9 relative (float64 arithmetic on the same integers in another order)."""
import json
import os
import re

import numpy as np
import pytest

from tests import neighbours_ref as NR
from tests.train_launch import launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 10
EXACT = ("classes_above_heldout", "classes_compared", "classes_used", "left_out", "loo_rows", "rejected_real", "rejected_heldout", "rejected_generated")
RATIOS = ("copy_rate", "copy_rate_heldout", "loo_1nn_accuracy", "loo_1nn_accuracy_real", "loo_1nn_accuracy_generated",
          "intra_class_loo_1nn_accuracy", "nearest_rmse_median", "nearest_rmse_median_heldout")
ARRAYS = ("copy_rate_per_class", "copy_rate_heldout_per_class", "loo_1nn_accuracy_per_class")


def _noisy(rs, x):
    return np.clip(np.rint(x.astype(np.float64) + 2.0 * rs.randn(*x.shape)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def world():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from rcgan_amd import neighbours as nb
    T, lt = D.synthetic_cifar(3000, 1234, "templates")
    H, lh = D.synthetic_cifar(600, 1235, "templates")
    F, lf = D.synthetic_cifar(600, 1236, "templates")
    rs = np.random.RandomState(7)
    pick = np.sort(rs.permutation(len(T))[:600])
    C, lc = _noisy(rs, T[pick]), lt[pick]
    one = D.template_images(np.random.RandomState(33), np.arange(K)).astype(np.uint8)
    lab = np.arange(600) % K
    sets = dict(fresh=(F, lf), copies=(C, lc), half=(np.concatenate([F[:300], C[:300]]), np.concatenate([lf[:300], lc[:300]])),
                collapsed=(_noisy(rs, one[lab]), lab))
    real = NR.prepare(T, lt, H, lh, K)
    ev = nb.NeighbourEvaluator(K)
    ev.prepare_real(T, lt, H, lh)
    w = dict(nb=nb, ev=ev, T=T, lt=lt, H=H, lh=lh, sets=sets, real=real, pick=pick,
             want={k: NR.evaluate(T, lt, H, lh, g, lg, K, real) for k, (g, lg) in sets.items()},
             got={k: ev.evaluate(g, lg) for k, (g, lg) in sets.items()})
    yield w
    ev.close()


def same_numbers(got, want):
    assert np.array_equal(got["nearest_index"], want["nearest_index"]) and np.array_equal(got["nearest_dist2"], want["nearest_dist2"])
    for key in EXACT:
        assert got[key] == want[key], key
    for key in RATIOS:
        assert got[key] == pytest.approx(want[key], rel=1e-12, nan_ok=True), key
    for key in ARRAYS:
        assert np.allclose(got[key], want[key], rtol=1e-12, atol=0, equal_nan=True), key
    assert got["nn_distance_z"] == pytest.approx(want["nn_distance_z"], rel=1e-9, nan_ok=True)
    assert got["intra_class_nn_distance_z"] == pytest.approx(want["intra_class_nn_distance_z"], rel=1e-9, nan_ok=True)
    assert np.allclose(got["nn_distance_z_per_class"], want["nn_distance_z_per_class"], rtol=1e-9, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", ["fresh", "copies", "half", "collapsed"])
def test_the_evaluator_equals_the_brute_force_restatement(world, name):
    got, want = world["got"][name], world["want"][name]
    print("%s: copy rate %.4f (held out %.4f), z %.3f, intra-class z %.3f (%d classes), 1-NN accuracy %.4f (real %.4f, generated %.4f), "
          "intra-class %.4f, nearest rmse %.2f (held out %.2f)" % (
              name, got["copy_rate"], got["copy_rate_heldout"], got["nn_distance_z"], got["intra_class_nn_distance_z"], got["classes_used"],
              got["loo_1nn_accuracy"], got["loo_1nn_accuracy_real"], got["loo_1nn_accuracy_generated"], got["intra_class_loo_1nn_accuracy"],
              got["nearest_rmse_median"], got["nearest_rmse_median_heldout"]))
    same_numbers(got, want)
    json.dumps(world["nb"].json_ready(got))


def test_the_state_kept_for_the_real_set_equals_the_restatement(world):
    real, ref = world["ev"].real, world["real"]
    assert np.array_equal(real["rho"], ref["rho"]) and np.array_equal(real["rho_class"], ref["rho_c"])
    assert np.array_equal(real["d_H"], ref["h"][0]) and np.array_equal(real["t_H"], ref["h"][1])
    assert np.array_equal(real["d_H_class"], ref["hc"][0]) and np.array_equal(real["t_H_class"], ref["hc"][1])
    assert (real["rho"] >= 0).all() and (real["rho_class"] >= real["rho"]).all()
    assert (world["lt"][real["t_H_class"]] == world["lh"]).all()


def test_the_numbers_separate_a_fresh_draw_from_copies_and_from_a_collapsed_set(world):
    fresh, copies, half, collapsed = (world["got"][k] for k in ("fresh", "copies", "half", "collapsed"))
    assert abs(fresh["nn_distance_z"]) < 4 and abs(fresh["copy_rate"] - fresh["copy_rate_heldout"]) < 0.08
    assert abs(fresh["loo_1nn_accuracy"] - 0.5) < 0.05
    assert copies["copy_rate"] > 0.9 and copies["nn_distance_z"] < -10 and copies["loo_1nn_accuracy"] < 0.45
    assert (copies["nearest_index"] == world["pick"]).all()                   # every copy finds the image it was made from
    assert fresh["copy_rate"] < half["copy_rate"] < copies["copy_rate"] and copies["nn_distance_z"] < half["nn_distance_z"] < -10
    assert collapsed["loo_1nn_accuracy_generated"] > 0.95
    assert copies["classes_above_heldout"] == K and copies["intra_class_nn_distance_z"] < -3


def test_small_classes_are_left_out_and_rows_with_a_foreign_label_are_counted(world):
    ev, (G, lg) = world["ev"], world["sets"]["fresh"]
    lg = lg.copy()
    rows3 = np.flatnonzero(lg == 3)
    lg[rows3[19:]] = K + 2                                           # class 3 keeps 19 rows: below the 20 its z needs
    lg[np.flatnonzero(lg == 5)[:4]] = -1
    got = ev.evaluate(G, lg)
    assert got["left_out"] == [3] and got["classes_used"] == K - 1 and np.isnan(got["nn_distance_z_per_class"][3])
    assert got["rejected_generated"] == len(rows3) - 19 + 4 and got["rejected_real"] == 0
    dropped = (lg < 0) | (lg >= K)
    assert (got["nearest_index"][dropped] == -1).all() and (got["nearest_index"][~dropped] >= 0).all()
    assert not np.isnan(got["copy_rate_per_class"]).any() and got["classes_compared"] == K
    same_numbers(got, NR.evaluate(world["T"], world["lt"], world["H"], world["lh"], G, lg, K, world["real"]))
    json.dumps(world["nb"].json_ready(got))


def test_nearest_takes_host_arrays_in_the_callers_order(world):
    nb, ev = world["nb"], world["ev"]
    rs = np.random.RandomState(9)
    q, ql = world["sets"]["half"][0][:200], world["sets"]["half"][1][:200].copy()
    r, rl = world["T"][:500], world["lt"][:500].copy()
    ql[7], rl[11] = 99, -2
    for per_class, exclude in ((False, False), (True, False)):
        d, j = nb.nearest(ev.ctx, q, ql, r, rl, per_class=per_class, exclude_same=exclude, n_classes=K)
        wd, wj = NR.nearest(q, ql, r, rl, K, per_class, exclude)
        assert np.array_equal(d, wd) and np.array_equal(j, wj), (per_class, exclude)
    for per_class in (False, True):
        d, j = nb.nearest(ev.ctx, r, rl, None, None, per_class=per_class, exclude_same=True, n_classes=K)
        wd, wj = NR.nearest(r, rl, r, rl, K, per_class, True)
        assert np.array_equal(d, wd) and np.array_equal(j, wj) and d[11] == -1 and (j != np.arange(len(r))).all()


def test_the_stand_alone_tool_prints_the_evaluators_numbers_as_one_json_line(world, tmp_path, capsys):
    nb = world["nb"]
    paths = [os.path.join(str(tmp_path), n + ".npz") for n in ("real", "heldout", "generated")]
    G, lg = world["sets"]["half"]
    np.savez(paths[0], images=world["T"], labels=world["lt"])
    np.savez(paths[1], images=world["H"].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), labels=world["lh"])        # (both layouts are taken)
    np.savez(paths[2], images=G, labels=lg)
    nb.main(["--real", paths[0], "--heldout", paths[1], "--generated", paths[2]])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r, got = json.loads(line[0]), world["got"]["half"]
    for key in ("copy_rate", "copy_rate_heldout", "nn_distance_z", "intra_class_nn_distance_z", "loo_1nn_accuracy", "loo_1nn_accuracy_real",
                "loo_1nn_accuracy_generated", "nearest_rmse_median"):
        assert r[key] == got[key], key
    assert r["nearest_index"] == got["nearest_index"].tolist() and r["classes_used"] == K and r["left_out"] == []


# ------------------------------------------------------------------------------------------------------------- command line
def _train(tmp_path, name, extra):
    return launch(tmp_path, extra, name)[0]


def test_training_logs_the_three_lines_at_every_period_and_at_the_end_and_writes_the_picture(tmp_path):
    text = _train(tmp_path, "n1", ["--neighbours_freq", "2", "--neighbours_samples", "200", "--neighbours_real_samples", "2000"])
    num = r"(-?[\d.]+(?:e[-+]?\d+)?|nan)"
    copy = re.findall(r"INFO\s+copy_rate: %s \(held-out %s\)$" % (num, num), text, flags=re.M)
    z = re.findall(r"INFO\s+nn_distance_z: %s, intra-class %s \((\d+) of 10 classes\)$" % (num, num), text, flags=re.M)
    acc = re.findall(r"INFO\s+loo_1nn_accuracy: %s \(real %s, generated %s\)$" % (num, num, num), text, flags=re.M)
    assert len(copy) == len(z) == len(acc) == 3, text[-3000:]                      # iterations 2 and 4, and the end of training
    assert all(0.0 <= float(a) <= 1.0 and 0.0 <= float(b) <= 1.0 for a, b in copy) and len({b for _, b in copy}) == 1
    assert all(0.0 <= float(a) <= 1.0 for row in acc for a in row)
    assert len(re.findall(r"neighbours real set: 2000 training images, 10000 held-out images", text)) == 1
    from PIL import Image
    for name in ("neighbours_1.png", "neighbours_3.png", "neighbours_final.png"):
        assert Image.open(os.path.join(str(tmp_path), "n1", name)).size == (20 * 32, 10 * 32)            # 100 pairs of 32 x 32 images


def test_training_without_the_flag_logs_none_of_the_lines(tmp_path):
    text = _train(tmp_path, "n0", [])
    assert not re.search(r"copy_rate|nn_distance_z|loo_1nn_accuracy|neighbours", text)
    assert not [f for f in os.listdir(os.path.join(str(tmp_path), "n0")) if f.startswith("neighbours")]
