"""The sliced Wasserstein distance without a GPU: the float64 restatement (tests/swd_ref.py) against facts that hold by construction
(the pyramid reconstructs the image, closed forms in one dimension, the lattice sizes), the orderings the number exists for on the
inputs the GPU test reuses, the library's exports and argument checks, and the schedule's sixth row on a stub evaluator."""
import ctypes as C
import logging

import numpy as np
import pytest

import rcgan_amd  # noqa: F401
from rcgan_amd import _lib, metrics, swd, train_cifar
from rcgan_amd.cifar import Z_DIM
from tests import swd_ref as SR

K, PER_CLASS, N_DIR = 4, 32, 128


def templates(seed, labels):
    from rcgan_amd import data as DT
    rows = DT.template_images(np.random.RandomState(seed), np.asarray(labels), n_classes=10).astype(np.uint8)
    return rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)


def world_inputs():
    """The image sets of the ordering tests (CPU and GPU): a real set of 64 per class, a second draw of 32 per class, the same draw
    under labels shuffled across classes, one image per class plus noise of sigma 2, and the draw blurred once (down then up)."""
    labels = np.random.RandomState(5).permutation(np.repeat(np.arange(K), PER_CLASS))
    real_labels = np.random.RandomState(6).permutation(np.repeat(np.arange(K), 2 * PER_CLASS))
    rs = np.random.RandomState(7)
    draw = templates(32, labels)
    one = templates(33, np.arange(K))
    collapsed = np.clip(np.rint(one[labels].astype(np.float64) + 2.0 * rs.randn(len(labels), 32, 32, 3)), 0, 255).astype(np.uint8)
    blurred = np.clip(np.rint(SR.up(SR.down(draw))), 0, 255).astype(np.uint8)
    return dict(real=templates(31, real_labels), real_labels=real_labels, labels=labels, draw=draw, shuffled_labels=rs.permutation(labels),
                collapsed=collapsed, blurred=blurred)


def orderings(clean, shuffled, collapsed, blurred):
    """The four orderings on results of ``SR.evaluate`` (or the evaluator's, mapped to the same keys)."""
    mean = lambda r: np.nanmean(r["per_class"], axis=0)
    assert mean(shuffled).mean() > 1.3 * mean(clean).mean()                      # label mixing: seen per class ...
    assert np.array_equal(shuffled["pooled"], clean["pooled"])                   # ... and invisible to the pooled value, bit for bit
    assert (mean(collapsed) > 1.5 * mean(clean)).all()                           # a collapsed class: at every level
    assert mean(blurred)[0] > 1.3 * mean(clean)[0]                               # lost sharpness: at the fine level


def test_the_pyramid_reconstructs_the_image():
    rs = np.random.RandomState(0)
    for shape in ((3, 32, 32, 3), (2, 28, 28, 1), (2, 28, 32, 3)):
        x = rs.randint(0, 256, size=shape).astype(np.uint8)
        l0, l1, l2 = SR.pyramid(x)
        assert l1.shape[1:3] == (shape[1] // 2, shape[2] // 2) and l2.shape[1:3] == (shape[1] // 4, shape[2] // 4)
        assert np.abs(l0 + SR.up(l1 + SR.up(l2)) - x).max() <= 1e-12
    flat = np.full((1, 32, 32, 3), 77, np.uint8)
    l0, l1, l2 = SR.pyramid(flat)
    assert not l0.any() and not l1.any() and (l2 == 77).all()                    # the taps sum to one under the mirror boundary too


def test_the_boundary_rule_and_the_lattices():
    assert SR._mirror(np.array([-2, -1, 0, 6, 7, 8]), 7).tolist() == [2, 1, 0, 6, 5, 4]
    assert [len(SR.lattice(s, st)) ** 2 for s, st in ((32, 4), (16, 2), (8, 1), (28, 4), (14, 2), (7, 1))] == [49, 25, 4, 36, 16, 1]
    assert [swd.positions(32, 32, l) for l in range(3)] == [49, 25, 4] and [swd.positions(28, 32, l) for l in range(3)] == [42, 20, 2]
    x = np.arange(2 * 8 * 8 * 3).reshape(2, 8, 8, 3).astype(np.float64)
    d = SR.descriptors(x, 1)
    assert d.shape == (2, 4, 147) and np.array_equal(d[1, 3].reshape(7, 7, 3), x[1, 1:8, 1:8, :])      # (dy, dx, channel), positions row-major


def test_the_distance_of_a_set_to_itself_is_zero_and_the_distance_is_symmetric():
    w = world_inputs()
    dirs = swd.directions(16, 3)
    a, b = w["draw"][:12], w["real"][:12]
    assert not SR.swd(a, a, dirs).any()
    assert np.array_equal(SR.swd(a, b, dirs), SR.swd(b, a, dirs))
    assert (SR.swd(a, b, dirs) > 0).all()


def test_one_dimensional_closed_forms():
    rs = np.random.RandomState(1)
    p = rs.randn(1, 50)
    assert SR.sliced(p, p[:, ::-1] + 0.25) == pytest.approx(250.0, rel=1e-12)     # a shift by t: W1 = |t|, whatever the order
    a, b = np.array([[0.0, 1.0] * 5]), np.array([[0.5, 3.0] * 5])                 # two-point sets: the quantiles pair up
    assert SR.sliced(a, b) == pytest.approx(1e3 * 0.5 * (0.5 + 2.0), rel=1e-12)
    a, b = np.array([[0.0] * 6 + [1.0] * 2]), np.array([[0.0] * 2 + [1.0] * 6])  # masses 3/4, 1/4 against 1/4, 3/4 at distance 1
    assert SR.sliced(a, b) == pytest.approx(500.0, rel=1e-12)


def test_directions_are_unit_vectors_from_a_private_stream():
    state = np.random.get_state()[1].copy()
    d = swd.directions(8, 3)
    assert d.shape == (3, 8, 147) and d.dtype == np.float32
    assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(axis=2)) - 1).max() < 1e-6
    assert np.array_equal(d, swd.directions(8, 3)) and np.array_equal(np.random.get_state()[1], state)


def test_the_four_orderings_hold_in_the_restatement():
    w = world_inputs()
    dirs = swd.directions(N_DIR, 3)
    ev = lambda x, y: SR.evaluate(w["real"], w["real_labels"], x, y, K, dirs)
    clean, shuffled = ev(w["draw"], w["labels"]), ev(w["draw"], w["shuffled_labels"])
    collapsed, blurred = ev(w["collapsed"], w["labels"]), ev(w["blurred"], w["labels"])
    for name, r in (("clean", clean), ("shuffled", shuffled), ("collapsed", collapsed), ("blurred", blurred)):
        print("%-9s pooled %s, per-class mean %s, floor %s" % (name, np.round(r["pooled"], 1), np.round(np.nanmean(r["per_class"], axis=0), 1),
                                                              np.round(np.nanmean(r["floor_per_class"], axis=0), 1)))
    orderings(clean, shuffled, collapsed, blurred)
    assert clean["counts"].tolist() == [PER_CLASS] * K
    # the floor is the clean draw's peer: the same distribution at the same count
    assert np.abs(np.log(np.nanmean(clean["per_class"], axis=0) / np.nanmean(clean["floor_per_class"], axis=0))).max() < np.log(1.6)


def test_the_library_exports_the_four_calls_and_refuses_them_without_a_context():
    lib = _lib.load()
    for name in ("rcgan_swd_moments", "rcgan_swd_project", "rcgan_sort_rows_f32", "rcgan_absdiff_rowsum"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and hasattr(_lib.load("f16"), name)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rcgan_swd_moments(None, 1, 32, 32, 3, 0, 4, 1, p, p, p, p) == _lib.EINVALID_ARG
    assert lib.rcgan_swd_project(None, 1, 32, 32, 3, 0, 4, 1, p, p, p, 1, p, 64, p) == _lib.EINVALID_ARG
    assert lib.rcgan_sort_rows_f32(None, 1, 2, p) == _lib.EINVALID_ARG
    assert lib.rcgan_absdiff_rowsum(None, 1, 2, 1, p, p, p, p) == _lib.EINVALID_ARG


# ------------------------------------------------------------------------------------------------------------------ the schedule
RESULT = dict(swd=30.0, floor_swd=20.0, intra_class_swd=40.0, intra_class_swd_se=2.0, classes_used=9, floor_intra_class_swd=25.0,
              swd_levels=[1.0, 2.0, 3.0], intra_class_swd_levels=[4.0, 5.0, 6.0], floor_swd_levels=[0.5, 1.5, 2.5],
              floor_intra_class_swd_levels=[3.5, 4.5, 5.5])


class World:
    def __init__(self, monkeypatch, caplog, argv):
        self.events, self.sampled, self.plotted = [], [], []
        world = self

        class Evaluator:
            def __init__(self, n_classes, **kw):
                world.events.append(("build", "swd", kw))

            def prepare_real(self, images, labels):
                world.events.append(("prepare", "swd", len(images)))

            def evaluate(self, images, labels):
                world.events.append(("evaluate", "swd", np.array(images).shape))
                return RESULT

            def close(self):
                world.events.append(("close", "swd"))

        class Other(Evaluator):
            def __init__(self, n_classes, **kw):
                world.events.append(("build", "msssim", kw))

            def prepare_real(self, images, labels):
                return dict(intra_class_msssim=0.3)

            def evaluate(self, images, labels):
                world.events.append(("evaluate", "msssim", np.array(images).shape))
                return dict(msssim=0.4, intra_class_msssim=0.5, intra_class_msssim_se=0.01, intra_class_msssim_real=0.3, left_out=[], undefined=[],
                            classes_above_real=2, classes_compared=10)

            def close(self):
                pass

        from rcgan_amd import msssim
        monkeypatch.setattr(swd, "SwdEvaluator", Evaluator)
        monkeypatch.setattr(msssim, "MsssimEvaluator", Other)
        caplog.set_level(logging.INFO)
        caplog.clear()
        self.caplog = caplog
        self.FLAGS = train_cifar.define_flags().parse(argv)
        metrics.check_flags(self.FLAGS)
        self.rs, self.twin = np.random.RandomState(5), np.random.RandomState(5)
        self.ev = metrics.Evaluations(self.FLAGS, 10, 0, "/run", self.sample, self.rs, self, np.zeros((100, Z_DIM), np.float32),
                                      train_cifar.grid_labels(10), lambda: (np.zeros((64, 3072), np.uint8), np.arange(64) % 10), lambda: None)

    def sample(self, labels, z):
        self.sampled.append(z)
        return np.zeros((len(labels), 3072), np.float32)

    def plot(self, name, value):
        self.plotted.append(name)

    def lines(self, starts=""):
        return [r.getMessage() for r in self.caplog.records if r.getMessage().startswith(starts)]


def test_the_swd_row_is_the_sixth_fires_at_its_period_and_runs_last(monkeypatch, caplog):
    assert [mt.prefix for mt in metrics.METRICS] == ["frechet", "prdc", "kid", "msssim", "neighbours", "swd"]
    assert metrics.METRICS[-1].features is False and [e[0] for e in metrics.METRICS[-1].extra] == ["swd_directions"]
    w = World(monkeypatch, caplog, ["--swd_freq", "2", "--swd_samples", "200", "--swd_real_samples", "40", "--swd_directions", "16",
                                    "--msssim_freq", "2", "--msssim_samples", "100"])
    for iteration in range(3):
        w.ev.run(iteration)
    assert [e[1] for e in w.events if e[0] == "evaluate"] == ["msssim", "swd"]                         # iteration 1 only; swd last
    assert ("build", "swd", dict(directions=16, device=0)) in w.events and ("prepare", "swd", 40) in w.events
    assert w.lines("swd real set") == ["swd real set: 40 images, 16 directions per level"]
    assert [l for l in w.lines() if l.startswith(("swd", "intra_class_swd"))][1:] == [
        "swd: 30.0, floor 20.0", "intra_class_swd: 40.0 +- 2.0 (9 of 10 classes), floor 25.0",
        "swd_level_0: 1.0, intra-class 4.0, floors 0.5, 3.5", "swd_level_1: 2.0, intra-class 5.0, floors 1.5, 4.5",
        "swd_level_2: 3.0, intra-class 6.0, floors 2.5, 5.5"]
    assert w.plotted[-2:] == ["swd", "intra_class_swd"]
    assert len(w.sampled) == 3                                                                          # 1 draw for msssim, 2 for swd
    w.ev.finish(None)
    w.ev.close()
    assert ("close", "swd") in w.events and w.lines("finished calculating")[-1] == "finished calculating sliced wasserstein distance."


def test_with_the_flag_off_nothing_is_built_logged_or_drawn(monkeypatch, caplog):
    w = World(monkeypatch, caplog, ["--swd_samples", "200"])
    assert w.FLAGS.swd_freq == 0 and w.FLAGS.swd_directions == 128
    for iteration in range(4):
        w.ev.run(iteration)
    w.ev.finish(None)
    w.ev.close()
    assert w.events == [] and w.lines() == [] and w.sampled == [] and w.plotted == []
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(w.rs.get_state(), w.twin.get_state()))


@pytest.mark.parametrize("argv", [["--swd_freq", "1", "--swd_directions", "0"], ["--swd_freq", "1", "--swd_directions", "1025"],
                                  ["--swd_freq", "-1"], ["--swd_freq", "1", "--swd_samples", "50"]])
def test_bad_flags_are_refused(argv):
    with pytest.raises(ValueError):
        metrics.check_flags(train_cifar.define_flags().parse(argv))
