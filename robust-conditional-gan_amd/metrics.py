"""The schedule of the sample-quality metrics of a training run: Frechet distance (frechet.py), k-NN precision / recall / density /
coverage (manifold.py), kernel distance (kid.py), intra-class MS-SSIM (msssim.py), pixel-space nearest neighbours (neighbours.py), the
sliced Wasserstein distance on Laplacian-pyramid patches (swd.py) and the radial power-spectrum distance (spectrum.py): seven in all.

``SCHEDULE`` (``METRICS``, the six rows that came first, and behind them ``SPECTRUM``) holds, per metric and in the order they run,
what differs between them: its flags, whether it reads the label classifier's
features, how its evaluator is built and prepared on the real set, and how a result becomes log lines and plot values.  Everything
else is said once, in ``Evaluations``: the periods, the balanced generated samples drawn from the run's private stream, the real sets
(read once), the one LabelClassifier the feature metrics share, and the order of closing.  numpy only at import; an evaluator module
is imported when its metric first fires."""
import collections
import logging
import os

import numpy as np

from .evaluators import permuted_labels

# prefix: of the flags --<prefix>_freq / _samples / _real_samples; title: '... calculating <title>.'; help: of those three flags;
# extra: ((flag, default, help, lowest, highest or None, the bound in words), ...); features: reads the label classifier's features;
# prepare(E, rx, ry, ...) -> (the evaluator after prepare_real on that slice of the training set, the log line of the real set) --
# a feature metric is also given clf, the shared classifier, and owner, 'of its own' if it is the one that calibrates it else 'shared';
# report(result, n_classes, FLAGS) -> (log lines, ((plot name, value), ...)); after(E, evaluator, iteration): optional, runs last
Metric = collections.namedtuple("Metric", "prefix title help extra features prepare report after")


def _prepare_frechet(E, rx, ry, clf, owner):
    from . import frechet as FR
    ev = FR.FrechetEvaluator(E.n_classes, asset=E.FLAGS.label_classifier, device=E.device, clf=clf)
    ev.prepare_real(rx, ry, cache_path=os.path.join(E.dir, FR.CACHE_NAME))
    return ev, 'frechet real statistics: {} images, {}'.format(len(rx), 'reused from ' + FR.CACHE_NAME if ev.reused else 'computed')


def _report_frechet(r, K, FLAGS):
    return (['frechet_distance: {}'.format(r["frechet_distance"]),
             'intra_class_frechet_distance: {} ({} of {} classes)'.format(r["intra_class_frechet_distance"], r["classes_used"], K)],
            [('frechet_distance', r["frechet_distance"]), ('intra_class_frechet_distance', r["intra_class_frechet_distance"])])


def _prepare_manifold(E, rx, ry, clf, owner):
    from . import manifold as MF
    ev = MF.ManifoldEvaluator(E.n_classes, k=E.FLAGS.prdc_k, asset=E.FLAGS.label_classifier, device=E.device, clf=clf)
    ev.prepare_real(rx, ry)
    return ev, 'manifold real set: {} images, k = {}, label classifier {}'.format(len(rx), E.FLAGS.prdc_k, owner)


def _report_manifold(r, K, FLAGS):
    from .manifold import METRICS as PRDC
    lines = ['manifold_{}: {}'.format(name, r[name]) for name in PRDC]
    lines += ['intra_class_manifold_{}: {} ({} of {} classes)'.format(name, r["intra_class_" + name], r["classes_used"], K) for name in PRDC]
    return lines, [pair for name in PRDC for pair in (('manifold_' + name, r[name]), ('intra_class_manifold_' + name, r["intra_class_" + name]))]


def _prepare_kid(E, rx, ry, clf, owner):
    from . import kid as KD
    ev = KD.KernelDistanceEvaluator(E.n_classes, subset_size=E.FLAGS.kid_subset_size, asset=E.FLAGS.label_classifier, device=E.device, clf=clf)
    ev.prepare_real(rx, ry)
    return ev, 'kernel distance real set: {} images, label classifier {}'.format(len(rx), owner)


def _report_kid(r, K, FLAGS):
    return (['kernel_distance: {}'.format(r["kernel_distance"]),
             'intra_class_kernel_distance: {} +- {} ({} of {} classes)'.format(
                 r["intra_class_kernel_distance"], r["intra_class_kernel_distance_se"], r["classes_used"], K),
             'kernel_distance_subsets: {} +- {} ({} of size {})'.format(r["subset_mean"], r["subset_std"], r["subsets"], FLAGS.kid_subset_size)],
            [('kernel_distance', r["kernel_distance"]), ('intra_class_kernel_distance', r["intra_class_kernel_distance"]),
             ('kernel_distance_subsets', r["subset_mean"])])


def _prepare_msssim(E, rx, ry):
    from . import msssim as MS
    ev = MS.MsssimEvaluator(E.n_classes, pairs=E.FLAGS.msssim_pairs, device=E.device)
    real = ev.prepare_real(rx, ry)
    return ev, 'msssim real set: {} images, {} pairs per class, intra-class {}'.format(len(rx), E.FLAGS.msssim_pairs, real["intra_class_msssim"])


def _report_msssim(r, K, FLAGS):
    used = K - len(r["left_out"]) - len(r["undefined"])
    return (['msssim: {}'.format(r["msssim"]),
             'intra_class_msssim: {} +- {} ({} of {} classes), real {}'.format(
                 r["intra_class_msssim"], r["intra_class_msssim_se"], used, K, r["intra_class_msssim_real"]),
             'msssim_classes_above_real: {} of {}'.format(r["classes_above_real"], r["classes_compared"])],
            [('msssim', r["msssim"]), ('intra_class_msssim', r["intra_class_msssim"]), ('msssim_classes_above_real', r["classes_above_real"])])


def _prepare_neighbours(E, rx, ry):
    from . import neighbours as NB
    ev = NB.NeighbourEvaluator(E.n_classes, device=E.device)
    hx, hy = E.real_set("heldout")
    real = ev.prepare_real(rx, ry, hx, hy)
    return ev, 'neighbours real set: {} training images, {} held-out images, held-out copy rate {}'.format(
        len(rx), len(hx), real["copy_rate_heldout"])


def _report_neighbours(r, K, FLAGS):
    return (['copy_rate: {} (held-out {})'.format(r["copy_rate"], r["copy_rate_heldout"]),
             'nn_distance_z: {}, intra-class {} ({} of {} classes)'.format(r["nn_distance_z"], r["intra_class_nn_distance_z"], r["classes_used"], K),
             'loo_1nn_accuracy: {} (real {}, generated {})'.format(
                 r["loo_1nn_accuracy"], r["loo_1nn_accuracy_real"], r["loo_1nn_accuracy_generated"])],
            [('copy_rate', r["copy_rate"]), ('nn_distance_z', r["nn_distance_z"]), ('loo_1nn_accuracy', r["loo_1nn_accuracy"])])


def _neighbours_picture(E, ev, iteration):
    """neighbours_<iteration>.png: the fixed grid's samples, each beside its nearest training image."""
    from .host import save_images
    grid = ((E.sample(E.fixed_labels, E.fixed_noise) + 1.) * (255. / 2)).astype('int32').reshape((100, 32, 32, 3))
    _, nearest = ev.nearest_training_rows(grid)
    found = ev.real["images"][np.maximum(nearest, 0)].reshape((100, 32, 32, 3))          # (kept as NHWC rows by the evaluator)
    pairs = np.stack([np.clip(grid, 0, 255).astype(np.uint8), found], axis=1).reshape((200, 32, 32, 3))
    save_images(pairs, os.path.join(E.dir, 'neighbours_{}.png'.format(iteration)))


def _prepare_swd(E, rx, ry):
    from . import swd as SW
    ev = SW.SwdEvaluator(E.n_classes, directions=E.FLAGS.swd_directions, device=E.device)
    ev.prepare_real(rx, ry)
    return ev, 'swd real set: {} images, {} directions per level'.format(len(rx), E.FLAGS.swd_directions)


def _report_swd(r, K, FLAGS):
    return (['swd: {}, floor {}'.format(r["swd"], r["floor_swd"]),
             'intra_class_swd: {} +- {} ({} of {} classes), floor {}'.format(
                 r["intra_class_swd"], r["intra_class_swd_se"], r["classes_used"], K, r["floor_intra_class_swd"])] +
            ['swd_level_{}: {}, intra-class {}, floors {}, {}'.format(
                l, r["swd_levels"][l], r["intra_class_swd_levels"][l], r["floor_swd_levels"][l], r["floor_intra_class_swd_levels"][l])
             for l in range(3)],
            [('swd', r["swd"]), ('intra_class_swd', r["intra_class_swd"])])


def _prepare_spectrum(E, rx, ry):
    from . import spectrum as SP
    ev = SP.SpectrumEvaluator(E.n_classes, device=E.device)
    ev.prepare_real(rx, ry)
    return ev, 'spectrum real set: {} images'.format(len(rx))


def _report_spectrum(r, K, FLAGS):
    return (['spectral_distance: {} dB, floor {}'.format(r["spectral_distance"], r["floor_spectral_distance"]),
             'intra_class_spectral_distance: {} +- {} dB ({} of {} classes), floor {}'.format(
                 r["intra_class_spectral_distance"], r["intra_class_spectral_distance_se"], r["classes_used"], K,
                 r["floor_intra_class_spectral_distance"])] +
            ['{}: {} dB, intra-class {}'.format(name, r[name], r["intra_class_" + name])
             for name in ("high_frequency_db", "nyquist_db", "checkerboard_db")],
            [('spectral_distance', r["spectral_distance"]), ('floor_spectral_distance', r["floor_spectral_distance"]),
             ('intra_class_spectral_distance', r["intra_class_spectral_distance"]),
             ('floor_intra_class_spectral_distance', r["floor_intra_class_spectral_distance"]),
             ('high_frequency_db', r["high_frequency_db"]), ('nyquist_db', r["nyquist_db"]), ('checkerboard_db', r["checkerboard_db"])])


def _spectrum_curves(E, ev, iteration):
    """spectrum_<iteration>.npz: the real and the generated reduced spectra, pooled [c,B] and per class [K,c,B], to plot later."""
    np.savez(os.path.join(E.dir, 'spectrum_{}.npz'.format(iteration)), **ev.spectra())


METRICS = (
    Metric("frechet", "frechet distance",
           ("period (iterations) of the Frechet distance on the label classifier's features, pooled and "
            "per class against the clean training set; also taken at the end of training (0: off)",
            "generated samples per Frechet evaluation (hundreds), balanced over the classes",
            "real images behind the real-set statistics (0: the whole training set)"),
           (), True, _prepare_frechet, _report_frechet, None),
    Metric("prdc", "manifold precision and recall",
           ("period (iterations) of k-NN precision / recall / density / coverage on the label classifier's "
            "features, pooled and per class against the clean training set; also taken at the end of training (0: off)",
            "generated samples per precision / recall evaluation (hundreds), balanced over the classes",
            "real images behind the real manifold (0: the whole training set)"),
           (("prdc_k", 5, "the k of the k-nearest-neighbour radii (1..16)", 1, 16, "in 1..16"),),
           True, _prepare_manifold, _report_manifold, None),
    Metric("kid", "kernel distance",
           ("period (iterations) of the kernel distance (unbiased cubic-kernel MMD^2) on the label classifier's "
            "features, pooled and per class against the clean training set; also taken at the end of training (0: off)",
            "generated samples per kernel-distance evaluation (hundreds), balanced over the classes",
            "real images behind the kernel distance (0: the whole training set)"),
           (("kid_subset_size", 1000, "rows per subset of the kernel distance's mean +- std over subsets (at least 2)", 2, None, "at least 2"),),
           True, _prepare_kid, _report_kid, None),
    Metric("msssim", "intra-class msssim",
           ("period (iterations) of the intra-class MS-SSIM of the generated IMAGES (random pairs per class, "
            "beside the same number on the clean training set); also taken at the end of training (0: off)",
            "generated samples per MS-SSIM evaluation (hundreds), balanced over the classes",
            "real images behind the real MS-SSIM values (0: the whole training set)"),
           (("msssim_pairs", 1000, "image pairs per class, and of the pooled value (at least 1)", 1, None, "at least 1"),),
           False, _prepare_msssim, _report_msssim, None),
    Metric("neighbours", "nearest training images",
           ("period (iterations) of the pixel-space nearest-training-image metrics (copy rate, nearest-neighbour "
            "distance z, leave-one-out 1-NN accuracy: does the generator memorise?); also taken at the end of training (0: off)",
            "generated samples per nearest-neighbour evaluation (hundreds), balanced over the classes",
            "training images the neighbours are searched in (0: the whole training set)"),
           (), False, _prepare_neighbours, _report_neighbours, _neighbours_picture),
    Metric("swd", "sliced wasserstein distance",
           ("period (iterations) of the sliced Wasserstein distance on Laplacian-pyramid patches of the generated IMAGES, pooled "
            "and per class against the clean training set, beside its floor; also taken at the end of training (0: off)",
            "generated samples per sliced-Wasserstein evaluation (hundreds), balanced over the classes",
            "real images the distance is taken against (0: the whole training set)"),
           (("swd_directions", 128, "random directions per pyramid level (1..1024)", 1, 1024, "in 1..1024"),),
           False, _prepare_swd, _report_swd, None),
)

# the seventh row; the schedule walks SCHEDULE, METRICS keeps the six rows it has always named
SPECTRUM = Metric("spectrum", "radial power spectrum",
                  ("period (iterations) of the radial power-spectrum distance of the generated IMAGES (log-spectral distance, high-frequency, "
                   "Nyquist and checkerboard energy in dB), pooled and per class against the clean training set, beside its floor; also "
                   "taken at the end of training (0: off)",
                   "generated samples per power-spectrum evaluation (hundreds), balanced over the classes",
                   "real images the spectra are compared with (0: the whole training set)"),
                  (), False, _prepare_spectrum, _report_spectrum, _spectrum_curves)
SCHEDULE = METRICS + (SPECTRUM,)


def define_flags(f):
    for mt in SCHEDULE:
        f.DEFINE_integer(mt.prefix + "_freq", 0, mt.help[0])
        f.DEFINE_integer(mt.prefix + "_samples", 10000, mt.help[1])
        f.DEFINE_integer(mt.prefix + "_real_samples", 0, mt.help[2])
        for name, default, text, _, _, _ in mt.extra:
            f.DEFINE_integer(name, default, text)


def check_flags(FLAGS):
    for mt in SCHEDULE:
        freq, real = getattr(FLAGS, mt.prefix + "_freq"), getattr(FLAGS, mt.prefix + "_real_samples")
        inside = all(lo <= getattr(FLAGS, name) and (hi is None or getattr(FLAGS, name) <= hi) for name, _, _, lo, hi, _ in mt.extra)
        if freq < 0 or real < 0 or (freq > 0 and (getattr(FLAGS, mt.prefix + "_samples") < 100 or not inside)):
            raise ValueError('--{0}_freq and --{0}_real_samples must not be negative, --{0}_samples at least 100'.format(mt.prefix) +
                             ''.join(', --{} {}'.format(name, words) for name, _, _, _, _, words in mt.extra))


class Evaluations:
    """The metrics of one run (rank 0).  sample(labels, z) -> [n,3072] generator output in [-1, 1]; rs: the run's private
    RandomState, the latents' only source; fixed_noise / fixed_labels: the fixed sample grid; load_train / load_heldout: () ->
    (images [N,3072] CHW rows, CLEAN labels) of the training set and of real images outside it, each called at most once and only
    when a metric is about to prepare.  Nothing is built before a metric first fires."""

    def __init__(self, FLAGS, n_classes, device, directory, sample, rs, plot, fixed_noise, fixed_labels, load_train, load_heldout):
        self.FLAGS, self.n_classes, self.device, self.dir = FLAGS, n_classes, device, directory
        self.sample, self.rs, self.plot = sample, rs, plot
        self.fixed_noise, self.fixed_labels = fixed_noise, fixed_labels
        self.loaders, self.sets = dict(train=load_train, heldout=load_heldout), {}
        self.enabled = [mt for mt in SCHEDULE if getattr(FLAGS, mt.prefix + "_freq") > 0]
        # the feature metrics read ONE classifier, built here on first need and calibrated by the first enabled of them in table order
        self.calibrating = next((mt for mt in self.enabled if mt.features), None)
        self.clf = None
        self.evaluators = {}                             # prefix -> evaluator, prepare_real done

    def real_set(self, which):
        if which not in self.sets:
            self.sets[which] = self.loaders[which]()
        return self.sets[which]

    def classifier(self):
        if self.clf is None:
            from .eval_cifar import ASSET, LabelClassifier
            asset = self.FLAGS.label_classifier
            self.clf = LabelClassifier(self.device, asset=ASSET if asset is None else asset)
        return self.clf

    def evaluator(self, mt):
        if mt.prefix not in self.evaluators:
            if mt.features and mt is not self.calibrating:
                self.evaluator(self.calibrating)       # it calibrates, on its own real slice (or restores the Frechet cache's calibration)
            shared = dict(clf=self.classifier(), owner='of its own' if mt is self.calibrating else 'shared') if mt.features else {}
            rx, ry = self.real_set("train")
            n_real = getattr(self.FLAGS, mt.prefix + "_real_samples")
            n_real = n_real if n_real > 0 else len(rx)
            self.evaluators[mt.prefix], line = mt.prepare(self, rx[:n_real], ry[:n_real], **shared)
            logging.info(line)
            if len(self.evaluators) == len(self.enabled):
                self.sets.clear()                      # every evaluator keeps what it needs of the real sets
        return self.evaluators[mt.prefix]

    def balanced_samples(self, n, confusion_matrix=None):
        """n generated images (NHWC, raw pixel scale, int32) with their conditioning labels balanced over the classes; rcgan-u: the
        labels mapped through the learned matrix."""
        from .train_cifar import gen_acc_label_lists
        balanced = gen_acc_label_lists(self.n_classes, balanced=True)
        calls = [balanced[j % len(balanced)] for j in range(n // 100)]
        samples = [self.sample(labels, self.rs.normal(size=(100, self.fixed_noise.shape[1])).astype('float32')) for labels in calls]
        samples = ((np.concatenate(samples, axis=0) + 1.) * (255.99 / 2)).astype('int32').reshape((-1, 32, 32, 3))
        labels = np.concatenate(calls, axis=0)
        if confusion_matrix is not None:
            labels = permuted_labels(labels, confusion_matrix)
        return samples, labels

    def evaluate(self, mt, iteration, confusion_matrix=None):
        logging.info('starting calculating %s%s.' % ('min. permuted ' if confusion_matrix is not None else '', mt.title))
        ev = self.evaluator(mt)
        r = ev.evaluate(*self.balanced_samples(getattr(self.FLAGS, mt.prefix + "_samples"), confusion_matrix))
        lines, plots = mt.report(r, self.n_classes, self.FLAGS)
        for line in lines:
            logging.info(line)
        for name, value in plots:
            self.plot.plot(name, value)
        if mt.after is not None:
            mt.after(self, ev, iteration)
        logging.info('finished calculating %s.' % mt.title)

    def run(self, iteration):
        """Every metric whose period ends with this iteration, in table order."""
        for mt in self.enabled:
            freq = getattr(self.FLAGS, mt.prefix + "_freq")
            if iteration % freq == freq - 1:
                self.evaluate(mt, iteration)

    def finish(self, confusion_matrix=None):
        """Every enabled metric once more at the end of training; with the learned matrix: on the labels mapped through it."""
        for mt in self.enabled:
            self.evaluate(mt, 'final', confusion_matrix)

    def close(self):
        for mt in reversed(self.enabled):
            if mt.prefix in self.evaluators:
                self.evaluators.pop(mt.prefix).close()
        if self.clf is not None:
            self.clf.close()
            self.clf = None
