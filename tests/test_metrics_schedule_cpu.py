"""The training-side schedule of the five sample-quality metrics (rcgan_amd.metrics.Evaluations) on stub evaluators: which metric runs
when and in which order, what is prepared on which slice of the real set and in which order, what the private sample stream gives up,
the plot names, and what is closed.  No GPU: the evaluator classes, the LabelClassifier and the picture writer are replaced."""
import logging

import numpy as np
import pytest

import rcgan_amd  # noqa: F401
from rcgan_amd import eval_cifar, frechet, host, kid, manifold, metrics, msssim, neighbours, train_cifar
from rcgan_amd.cifar import Z_DIM

K, N_TRAIN, N_HELDOUT = 10, 64, 16
PERIODS = ["--frechet_freq", "2", "--prdc_freq", "4", "--kid_freq", "2", "--msssim_freq", "4", "--neighbours_freq", "2"]
SAMPLES = [a for p in ("frechet", "prdc", "kid", "msssim", "neighbours") for a in ("--%s_samples" % p, "200")]
TITLES = dict(frechet="frechet distance", prdc="manifold precision and recall", kid="kernel distance", msssim="intra-class msssim",
              neighbours="nearest training images")
# the plot.plot calls of one evaluation, written out from the training entry as it stood before the schedule existed
PLOTS = dict(frechet=["frechet_distance", "intra_class_frechet_distance"],
             prdc=["manifold_precision", "intra_class_manifold_precision", "manifold_recall", "intra_class_manifold_recall",
                   "manifold_density", "intra_class_manifold_density", "manifold_coverage", "intra_class_manifold_coverage"],
             kid=["kernel_distance", "intra_class_kernel_distance", "kernel_distance_subsets"],
             msssim=["msssim", "intra_class_msssim", "msssim_classes_above_real"],
             neighbours=["copy_rate", "nn_distance_z", "loo_1nn_accuracy"])
RESULTS = dict(
    frechet=dict(frechet_distance=1.0, intra_class_frechet_distance=2.0, classes_used=K),
    prdc=dict([(m, 0.5) for m in manifold.METRICS] + [("intra_class_" + m, 0.25) for m in manifold.METRICS], classes_used=K),
    kid=dict(kernel_distance=0.1, intra_class_kernel_distance=0.2, intra_class_kernel_distance_se=0.01, subset_mean=0.3, subset_std=0.02,
             subsets=3, classes_used=K),
    msssim=dict(msssim=0.4, intra_class_msssim=0.5, intra_class_msssim_se=0.01, intra_class_msssim_real=0.3, left_out=[], undefined=[1],
                classes_above_real=2, classes_compared=9),
    neighbours=dict(copy_rate=0.0, copy_rate_heldout=0.1, nn_distance_z=-1.0, intra_class_nn_distance_z=-2.0, classes_used=K,
                    loo_1nn_accuracy=0.6, loo_1nn_accuracy_real=0.5, loo_1nn_accuracy_generated=0.7))


class World:
    """One run of the schedule on stubs; ``events`` is everything the stubs saw, in order."""

    def __init__(self, monkeypatch, caplog, argv, seed=5):
        self.events, self.sampled, self.plotted, self.pictures = [], [], [], []
        self.loads = dict(train=0, heldout=0)
        self.train = (np.arange(N_TRAIN * 3072).reshape(N_TRAIN, 3072) % 251, np.arange(N_TRAIN) % K)
        self.heldout = (np.zeros((N_HELDOUT, 3072), np.uint8), np.arange(N_HELDOUT) % K)
        world = self

        class Classifier:
            def __init__(self, device, asset=None):
                world.events.append(("build", "classifier", asset))

            def close(self):
                world.events.append(("close", "classifier"))

        def stub(name):
            class Evaluator:
                reused = False

                def __init__(self, n_classes, clf=None, **kw):
                    assert n_classes == K
                    self.clf, self.kw = clf, kw
                    self.real = dict(images=np.zeros((N_TRAIN, 3072), np.uint8))
                    world.events.append(("build", name, clf))

                def prepare_real(self, images, labels, *heldout, **kw):
                    world.events.append(("prepare", name, np.array(images), np.array(labels), heldout, kw))
                    return dict(intra_class_msssim=0.3, copy_rate_heldout=0.1)

                def evaluate(self, images, labels):
                    world.events.append(("evaluate", name, np.array(images), np.array(labels)))
                    return RESULTS[name]

                def nearest_training_rows(self, images):
                    return np.zeros(len(images), np.int64), np.arange(len(images)) % N_TRAIN

                def close(self):
                    world.events.append(("close", name))
            return Evaluator

        monkeypatch.setattr(eval_cifar, "LabelClassifier", Classifier)
        for module, cls, name in ((frechet, "FrechetEvaluator", "frechet"), (manifold, "ManifoldEvaluator", "prdc"), (kid, "KernelDistanceEvaluator", "kid"),
                                  (msssim, "MsssimEvaluator", "msssim"), (neighbours, "NeighbourEvaluator", "neighbours")):
            monkeypatch.setattr(module, cls, stub(name))
        monkeypatch.setattr(host, "save_images", lambda images, path: self.pictures.append((np.array(images), path)))
        caplog.set_level(logging.INFO)
        caplog.clear()
        self.caplog = caplog
        self.FLAGS = train_cifar.define_flags().parse(argv)
        metrics.check_flags(self.FLAGS)
        self.rs, self.twin = np.random.RandomState(seed), np.random.RandomState(seed)
        self.fixed_noise = np.random.RandomState(1).normal(size=(100, Z_DIM)).astype("float32")
        self.fixed_labels = train_cifar.grid_labels(K)
        self.ev = metrics.Evaluations(self.FLAGS, K, 0, "/run", self.sample, self.rs, self, self.fixed_noise, self.fixed_labels,
                                      lambda: self.load("train"), lambda: self.load("heldout"))

    def load(self, which):
        self.loads[which] += 1
        return getattr(self, which)

    def sample(self, labels, z):
        self.sampled.append((np.array(labels), np.array(z)))
        return np.tanh(z[:, :1] + np.asarray(labels)[:, None] / K) * np.ones((1, 3072), np.float32)

    def plot(self, name, value):
        self.plotted.append(name)

    def lines(self, starts=""):
        return [r.getMessage() for r in self.caplog.records if r.getMessage().startswith(starts)]

    def of(self, kind, name=None):
        return [e for e in self.events if e[0] == kind and name in (None, e[1])]


def started(titles, prefix=""):
    return ["starting calculating %s%s." % (prefix, TITLES[t]) for t in titles]


ALL = ["frechet", "prdc", "kid", "msssim", "neighbours"]


def test_periods_order_loads_slices_stream_plots_and_close(monkeypatch, caplog):
    real = ["--frechet_real_samples", "30", "--prdc_real_samples", "40", "--msssim_real_samples", "1000"]
    w = World(monkeypatch, caplog, PERIODS + SAMPLES + real + ["--label_classifier", "some.npz"])
    for iteration in range(4):
        w.ev.run(iteration)
    w.ev.finish(None)
    # (a) which metric runs when, in table order
    assert w.lines("starting calculating") == started(["frechet", "kid", "neighbours"]) + started(ALL) + started(ALL)
    finished = [l.replace("finished", "starting") for l in w.lines("finished calculating")]
    assert finished == w.lines("starting calculating")
    assert [e[1] for e in w.of("evaluate")] == ["frechet", "kid", "neighbours"] + ALL + ALL
    # (b) each real set read once; each evaluator prepared once, on its own slice of the training set
    assert w.loads == dict(train=1, heldout=1)
    assert sorted(e[1] for e in w.of("prepare")) == sorted(ALL)
    for name, n in (("frechet", 30), ("prdc", 40), ("kid", N_TRAIN), ("msssim", N_TRAIN), ("neighbours", N_TRAIN)):
        (_, _, images, labels, heldout, kw), = w.of("prepare", name)
        assert np.array_equal(images, w.train[0][:n]) and np.array_equal(labels, w.train[1][:n]), name
        assert (len(heldout) == 2 and heldout[0] is w.heldout[0] and heldout[1] is w.heldout[1]) if name == "neighbours" else heldout == ()
        assert kw == (dict(cache_path="/run/" + frechet.CACHE_NAME) if name == "frechet" else {})
    assert w.lines("frechet real statistics") == ["frechet real statistics: 30 images, computed"]
    assert w.lines("manifold real set") == ["manifold real set: 40 images, k = 5, label classifier shared"]
    assert w.lines("kernel distance real set") == ["kernel distance real set: %d images, label classifier shared" % N_TRAIN]
    assert w.lines("msssim real set") == ["msssim real set: %d images, 1000 pairs per class, intra-class 0.3" % N_TRAIN]
    assert w.lines("neighbours real set") == ["neighbours real set: %d training images, %d held-out images, held-out copy rate 0.1" % (N_TRAIN, N_HELDOUT)]
    # one classifier, from the run's asset, handed to the three feature evaluators and to nobody else
    (_, _, asset), = w.of("build", "classifier")
    assert asset == "some.npz"
    built = {e[1]: e[2] for e in w.of("build") if e[1] != "classifier"}
    assert built["frechet"] is built["prdc"] is built["kid"] is w.ev.clf and built["msssim"] is None and built["neighbours"] is None
    # (d) the private stream: 2 draws of (100, Z_DIM) per evaluation of 200 samples, in evaluation order, and nothing else
    pictures = [i for i, (labels, z) in enumerate(w.sampled) if z is not None and np.array_equal(z, w.fixed_noise)]
    draws = [z for i, (labels, z) in enumerate(w.sampled) if i not in pictures]
    assert len(draws) == 2 * 13 and len(pictures) == 3
    for z in draws:
        assert z.dtype == np.float32 and np.array_equal(z, w.twin.normal(size=(100, Z_DIM)).astype("float32"))
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(w.rs.get_state(), w.twin.get_state()))
    balanced = train_cifar.gen_acc_label_lists(K, balanced=True)
    for e in w.of("evaluate"):
        assert e[2].shape == (200, 32, 32, 3) and e[2].dtype == np.int32 and np.array_equal(e[3], np.concatenate(balanced[:2]))
    # the evaluator sees what the sampler returned for those draws, scaled to raw pixels
    labels, z = [s for i, s in enumerate(w.sampled) if i not in pictures][0]
    want = ((np.tanh(z[:, :1] + labels[:, None] / K) * np.ones((1, 3072), np.float32) + 1.) * (255.99 / 2)).astype("int32").reshape(100, 32, 32, 3)
    assert np.array_equal(w.of("evaluate")[0][2][:100], want)
    # (e) the plot names and their order
    assert w.plotted == sum([PLOTS[t] for t in ["frechet", "kid", "neighbours"] + ALL + ALL], [])
    # the after-hook: one picture per evaluation of the nearest-neighbour metric
    assert [p for _, p in w.pictures] == ["/run/neighbours_1.png", "/run/neighbours_3.png", "/run/neighbours_final.png"]
    assert all(images.shape == (200, 32, 32, 3) and images.dtype == np.uint8 for images, _ in w.pictures)
    # (g) close: every evaluator, then the classifier, once
    w.ev.close()
    w.ev.close()
    closed = [e[1] for e in w.of("close")]
    assert sorted(closed[:-1]) == sorted(ALL) and closed[-1] == "classifier"


def test_the_log_lines_of_one_evaluation_of_each_metric(monkeypatch, caplog):
    w = World(monkeypatch, caplog, sum([["--%s_freq" % p, "1"] for p in ALL], []) + SAMPLES)
    w.ev.run(0)
    assert [l for l in w.lines() if "real s" not in l and "calculating" not in l] == [
        "frechet_distance: 1.0", "intra_class_frechet_distance: 2.0 (10 of 10 classes)",
        "manifold_precision: 0.5", "manifold_recall: 0.5", "manifold_density: 0.5", "manifold_coverage: 0.5",
        "intra_class_manifold_precision: 0.25 (10 of 10 classes)", "intra_class_manifold_recall: 0.25 (10 of 10 classes)",
        "intra_class_manifold_density: 0.25 (10 of 10 classes)", "intra_class_manifold_coverage: 0.25 (10 of 10 classes)",
        "kernel_distance: 0.1", "intra_class_kernel_distance: 0.2 +- 0.01 (10 of 10 classes)", "kernel_distance_subsets: 0.3 +- 0.02 (3 of size 1000)",
        "msssim: 0.4", "intra_class_msssim: 0.5 +- 0.01 (9 of 10 classes), real 0.3", "msssim_classes_above_real: 2 of 9",
        "copy_rate: 0.0 (held-out 0.1)", "nn_distance_z: -1.0, intra-class -2.0 (10 of 10 classes)", "loo_1nn_accuracy: 0.6 (real 0.5, generated 0.7)"]


@pytest.mark.parametrize("on, order, words", [
    # (c) the first enabled feature metric calibrates, on its own slice, before any other feature metric prepares
    (["frechet", "prdc", "kid"], ["frechet", "kid"], {"prdc": "shared", "kid": "shared"}),
    (["prdc", "kid"], ["prdc", "kid"], {"prdc": "of its own", "kid": "shared"}),
])
def test_the_first_enabled_feature_metric_prepares_before_one_that_fires_earlier(monkeypatch, caplog, on, order, words):
    periods = dict(frechet="4", prdc="4", kid="2")
    real = dict(frechet="20", prdc="30", kid="40")
    argv = sum([["--%s_freq" % p, periods[p], "--%s_real_samples" % p, real[p]] for p in on], []) + SAMPLES
    w = World(monkeypatch, caplog, argv)
    w.ev.run(1)                                                     # only the kernel distance fires
    assert w.lines("starting calculating") == started(["kid"])
    assert [e[1] for e in w.of("prepare")] == order and [e[1] for e in w.of("evaluate")] == ["kid"]
    assert [len(e[2]) for e in w.of("prepare")] == [int(real[p]) for p in order]
    assert len(w.of("build", "classifier")) == 1 and w.of("build", "classifier")[0][2] == eval_cifar.ASSET
    log = w.lines()
    if "frechet" in on:
        assert log[1:3] == ["frechet real statistics: 20 images, computed", "kernel distance real set: 40 images, label classifier shared"]
        assert not w.lines("manifold real set")                     # prepared only when it first fires
    else:
        assert log[1:3] == ["manifold real set: 30 images, k = 5, label classifier of its own", "kernel distance real set: 40 images, label classifier shared"]
    w.ev.run(3)
    assert [e[1] for e in w.of("prepare")] == order + [p for p in on if p not in order]
    for p, word in words.items():
        assert any(l.endswith("label classifier " + word) for l in w.lines({"prdc": "manifold", "kid": "kernel distance"}[p] + " real set")), p
    assert len(w.of("build", "classifier")) == 1 and w.loads == dict(train=1, heldout=0)


def test_with_every_metric_off_nothing_is_logged_built_or_loaded(monkeypatch, caplog):
    w = World(monkeypatch, caplog, SAMPLES)
    for iteration in range(4):
        w.ev.run(iteration)
    w.ev.finish(np.eye(K))
    w.ev.close()
    assert not w.ev.enabled and w.lines() == [] and w.events == [] and w.sampled == [] and w.plotted == [] and w.pictures == []
    assert w.loads == dict(train=0, heldout=0)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(w.rs.get_state(), w.twin.get_state()))


def test_finish_with_the_learned_matrix_permutes_the_labels_and_says_so(monkeypatch, caplog):
    w = World(monkeypatch, caplog, ["--kid_freq", "100", "--neighbours_freq", "100"] + SAMPLES)
    perm = np.roll(np.arange(K), 3)
    cm = np.full((K, K), 0.01)
    cm[np.arange(K), perm] = 0.9
    seen = []
    monkeypatch.setattr(metrics, "permuted_labels", lambda labels, matrix: (seen.append(matrix), frechet.permuted_labels(labels, matrix))[1])
    w.ev.finish(cm)
    assert w.lines("starting calculating") == started(["kid", "neighbours"], "min. permuted ")
    assert w.lines("finished calculating") == ["finished calculating kernel distance.", "finished calculating nearest training images."]
    balanced = np.concatenate(train_cifar.gen_acc_label_lists(K, balanced=True)[:2])
    assert len(seen) == 2 and all(m is cm for m in seen)
    for e in w.of("evaluate"):
        assert np.array_equal(e[3], perm[balanced])
    assert [np.array_equal(labels, b) for (labels, _), b in zip(w.sampled[:2], train_cifar.gen_acc_label_lists(K, balanced=True))] == [True, True]
    assert [p for _, p in w.pictures] == ["/run/neighbours_final.png"]
