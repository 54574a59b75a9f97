"""The seventh row of the metric schedule (rcgan_amd.metrics.SCHEDULE = METRICS + (SPECTRUM,): the radial power-spectrum distance) on stub evaluators: when
it fires and after whom, the slice it prepares on, its log lines and plot names, the curves it writes, and that with the flag at 0
its module is never imported.  No GPU."""
import logging
import subprocess
import sys
import os

import numpy as np

import rcgan_amd  # noqa: F401
from rcgan_amd import metrics, train_cifar
from rcgan_amd.cifar import Z_DIM

RESULT = dict(spectral_distance=3.0, floor_spectral_distance=0.4, intra_class_spectral_distance=3.5, intra_class_spectral_distance_se=0.2,
              floor_intra_class_spectral_distance=0.6, classes_used=9, high_frequency_db=-4.0, intra_class_high_frequency_db=-4.5,
              nyquist_db=1.0, intra_class_nyquist_db=1.5, checkerboard_db=8.0, intra_class_checkerboard_db=8.5)
CURVES = dict(real=np.ones((3, 24)), generated=np.full((3, 24), 2.0), real_per_class=np.ones((10, 3, 24)),
              generated_per_class=np.full((10, 3, 24), 2.0), ring_counts=np.arange(24))


class World:
    def __init__(self, monkeypatch, caplog, argv):
        from rcgan_amd import spectrum, swd
        self.events, self.sampled, self.plotted, self.saved = [], [], [], []
        world = self

        def stub(name, result):
            class Evaluator:
                def __init__(self, n_classes, **kw):
                    world.events.append(("build", name, kw))

                def prepare_real(self, images, labels):
                    world.events.append(("prepare", name, np.array(images), np.array(labels)))

                def evaluate(self, images, labels):
                    world.events.append(("evaluate", name, np.array(images).shape))
                    return result

                def spectra(self):
                    return CURVES

                def close(self):
                    world.events.append(("close", name))
            return Evaluator

        swd_result = dict(swd=30.0, floor_swd=20.0, intra_class_swd=40.0, intra_class_swd_se=2.0, classes_used=9, floor_intra_class_swd=25.0,
                          swd_levels=[1.0, 2.0, 3.0], intra_class_swd_levels=[4.0, 5.0, 6.0], floor_swd_levels=[0.5, 1.5, 2.5],
                          floor_intra_class_swd_levels=[3.5, 4.5, 5.5])
        monkeypatch.setattr(spectrum, "SpectrumEvaluator", stub("spectrum", RESULT))
        monkeypatch.setattr(swd, "SwdEvaluator", stub("swd", swd_result))
        monkeypatch.setattr(metrics.np, "savez", lambda path, **arrays: self.saved.append((path, arrays)))
        caplog.set_level(logging.INFO)
        caplog.clear()
        self.caplog = caplog
        self.FLAGS = train_cifar.define_flags().parse(argv)
        metrics.check_flags(self.FLAGS)
        self.train = (np.arange(64 * 3072).reshape(64, 3072) % 251, np.arange(64) % 10)
        self.rs, self.twin = np.random.RandomState(5), np.random.RandomState(5)
        self.ev = metrics.Evaluations(self.FLAGS, 10, 0, "/run", self.sample, self.rs, self, np.zeros((100, Z_DIM), np.float32),
                                      train_cifar.grid_labels(10), lambda: self.train, lambda: None)

    def sample(self, labels, z):
        self.sampled.append(z)
        return np.zeros((len(labels), 3072), np.float32)

    def plot(self, name, value):
        self.plotted.append((name, value))

    def lines(self, starts=""):
        return [r.getMessage() for r in self.caplog.records if r.getMessage().startswith(starts)]


def test_the_spectrum_row_is_the_seventh_and_fires_at_its_period_after_swd(monkeypatch, caplog):
    assert [mt.prefix for mt in metrics.SCHEDULE] == ["frechet", "prdc", "kid", "msssim", "neighbours", "swd", "spectrum"]
    assert metrics.SCHEDULE[:6] == metrics.METRICS and metrics.SCHEDULE[6] is metrics.SPECTRUM
    row = metrics.SCHEDULE[6]
    assert row.features is False and row.extra == () and row.after is not None
    w = World(monkeypatch, caplog, ["--spectrum_freq", "2", "--spectrum_samples", "200", "--spectrum_real_samples", "40",
                                    "--swd_freq", "2", "--swd_samples", "100"])
    for iteration in range(4):
        w.ev.run(iteration)
    assert [e[1] for e in w.events if e[0] == "evaluate"] == ["swd", "spectrum", "swd", "spectrum"]      # iterations 1 and 3
    assert ("build", "spectrum", dict(device=0)) in w.events
    (_, _, images, labels), = [e for e in w.events if e[:2] == ("prepare", "spectrum")]
    assert np.array_equal(images, w.train[0][:40]) and np.array_equal(labels, w.train[1][:40])          # its own slice
    assert w.lines("spectrum real set") == ["spectrum real set: 40 images"]
    assert [e[2] for e in w.events if e[:2] == ("evaluate", "spectrum")] == [(200, 32, 32, 3)] * 2
    own = [l for l in w.lines() if l.startswith(("spectral_distance", "intra_class_spectral_distance", "high_frequency_db", "nyquist_db",
                                                 "checkerboard_db"))]
    assert own[:5] == ["spectral_distance: 3.0 dB, floor 0.4",
                       "intra_class_spectral_distance: 3.5 +- 0.2 dB (9 of 10 classes), floor 0.6",
                       "high_frequency_db: -4.0 dB, intra-class -4.5", "nyquist_db: 1.0 dB, intra-class 1.5",
                       "checkerboard_db: 8.0 dB, intra-class 8.5"] and len(own) == 10
    assert w.plotted[2:9] == [("spectral_distance", 3.0), ("floor_spectral_distance", 0.4), ("intra_class_spectral_distance", 3.5),
                              ("floor_intra_class_spectral_distance", 0.6), ("high_frequency_db", -4.0), ("nyquist_db", 1.0),
                              ("checkerboard_db", 8.0)]
    assert [p for p, _ in w.saved] == ["/run/spectrum_1.npz", "/run/spectrum_3.npz"]
    assert sorted(w.saved[0][1]) == sorted(CURVES) and w.saved[0][1]["generated_per_class"] is CURVES["generated_per_class"]
    assert len(w.sampled) == 2 * (1 + 2)                                                                  # 1 draw for swd, 2 for spectrum
    w.ev.finish(None)
    w.ev.close()
    assert w.saved[-1][0] == "/run/spectrum_final.npz" and ("close", "spectrum") in w.events
    assert w.lines("finished calculating")[-1] == "finished calculating radial power spectrum."


def test_with_the_flag_off_nothing_is_built_logged_drawn_or_written(monkeypatch, caplog):
    w = World(monkeypatch, caplog, ["--spectrum_samples", "200"])
    assert w.FLAGS.spectrum_freq == 0 and w.FLAGS.spectrum_samples == 200 and w.FLAGS.spectrum_real_samples == 0
    for iteration in range(4):
        w.ev.run(iteration)
    w.ev.finish(None)
    w.ev.close()
    assert w.events == [] and w.lines() == [] and w.sampled == [] and w.plotted == [] and w.saved == []
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(w.rs.get_state(), w.twin.get_state()))


def test_with_the_flag_off_the_module_is_never_imported():
    """In a fresh interpreter: the schedule with another metric on and this one off runs without rcgan_amd.spectrum in sys.modules."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np\n"
            "import rcgan_amd\n"
            "from rcgan_amd import metrics, train_cifar, swd\n"
            "from rcgan_amd.cifar import Z_DIM\n"
            "class Ev:\n"
            "    def __init__(self, n_classes, **kw): pass\n"
            "    def prepare_real(self, x, y): pass\n"
            "    def evaluate(self, x, y): return dict(swd=1.0, floor_swd=1.0, intra_class_swd=1.0, intra_class_swd_se=1.0, classes_used=10,\n"
            "        floor_intra_class_swd=1.0, swd_levels=[1.0] * 3, intra_class_swd_levels=[1.0] * 3, floor_swd_levels=[1.0] * 3,\n"
            "        floor_intra_class_swd_levels=[1.0] * 3)\n"
            "    def close(self): pass\n"
            "swd.SwdEvaluator = Ev\n"
            "FLAGS = train_cifar.define_flags().parse(['--swd_freq', '1', '--swd_samples', '100'])\n"
            "metrics.check_flags(FLAGS)\n"
            "plot = type('P', (), dict(plot=staticmethod(lambda n, v: None)))\n"
            "E = metrics.Evaluations(FLAGS, 10, 0, '/run', lambda labels, z: np.zeros((len(labels), 3072), np.float32), np.random.RandomState(0), plot,\n"
            "                        np.zeros((100, Z_DIM), np.float32), train_cifar.grid_labels(10), lambda: (np.zeros((20, 3072), np.uint8), np.arange(20) % 10), lambda: None)\n"
            "E.run(0); E.finish(None); E.close()\n"
            "assert 'rcgan_amd.swd' in sys.modules\n"
            "print('spectrum imported:', 'rcgan_amd.spectrum' in sys.modules)\n")
    child = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    assert child.stdout.strip().splitlines()[-1] == "spectrum imported: False"


def test_bad_flags_are_refused():
    import pytest
    for argv in (["--spectrum_freq", "-1"], ["--spectrum_freq", "1", "--spectrum_samples", "50"], ["--spectrum_real_samples", "-3"]):
        with pytest.raises(ValueError):
            metrics.check_flags(train_cifar.define_flags().parse(argv))
