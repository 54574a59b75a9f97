"""Train the generated-label-accuracy classifier for a data set (``cifar10/run_label_classifier.sh``) and write the weight asset
that ``train_cifar.py --label_classifier PATH`` scores generated samples with.

Trains on the CLEAN training labels: a classifier trained on the corrupted ones would measure the label noise, not the generator.
The held-out set is scored under the evaluator's protocol (batches of 1000, every batch norm on the moments of its batch).

With only NOISY labels and a confusion matrix C (``cifar10/run_label_recovery.sh``): ``--loss forward`` trains on them with the
forward-corrected loss -log((softmax(z) . C)[label]) (Patrini et al. 2017), under which the soft-max estimates the clean posterior, so
the asset is still a drop-in for ``--label_classifier``; ``--recover_out`` then writes the recovered training labels.  The matrix is
``known`` (the one-coin matrix of ``--alpha``), a ``.npy`` file (for instance the matrix an RCGAN-U run learned), or ``estimate``:
a plain cross-entropy stage on the noisy labels, Patrini's anchor estimate from its soft-max over the training set, then the
forward-corrected run from a fresh initialisation.  ``--alpha`` below 1 corrupts the training labels once (a stand-in for labels
that arrive noisy); the clean ones are then kept for reporting only.

The label-noise flags and their checks, the corruption, matrix loading, the training loop and the writer of ``--recover_out`` are
``label_driver``'s, shared with ``train_mnist_classifier.py``.
"""
import logging
import os
import sys

import numpy as np

from . import data as D
from . import label_driver as V
from .host import Flags
from .train_cifar import DATA_DIR, dataset_setup


def define_flags():
    f = Flags()
    f.DEFINE_string("dataset", 'cifar', "Dataset [cifar, cifar100]")
    f.DEFINE_boolean("coarse_labels", False, "--dataset cifar100: the 20 coarse labels instead of the 100 fine ones")
    f.DEFINE_string("data_dir", DATA_DIR, "CIFAR-10 python batches (--dataset cifar100: the cifar-100-python directory)")
    f.DEFINE_boolean("synthetic", False, "train on the synthetic stand-in data instead of the files under --data_dir")
    f.DEFINE_string("synthetic_kind", 'uniform', "with --synthetic: [uniform] label-free noise images, [templates] class-pattern images")
    f.DEFINE_integer("synthetic_samples", 50000, "with --synthetic: size of the training set (the held-out set is a fifth of it)")
    f.DEFINE_integer("epochs", 160, "passes over the training set")
    f.DEFINE_integer("max_steps", 0, "if > 0: stop after this many steps (the learning-rate schedule then spans them)")
    f.DEFINE_integer("batch_size", 128, "batch size")
    f.DEFINE_float("lr", 0.1, "learning rate; divided by 10 at 50 % and at 75 % of the run")
    f.DEFINE_float("momentum", 0.9, "momentum")
    f.DEFINE_float("weight_decay", 1e-4, "L2 weight decay on the filters and the dense weight")
    f.DEFINE_boolean("nesterov", False, "Nesterov momentum")
    f.DEFINE_boolean("no_augment", False, "no random translation / mirror")
    f.DEFINE_integer("seed", 0, "seed of the initialisation and of the input pipeline")
    f.DEFINE_string("f32_matmul_precision", 'highest', "fp32 GEMMs [highest: fp32 matrix cores, high: split-bf16 matrix cores]")
    V.define_noise_flags(f, "K", "with --loss forward: [known] C_ALPHA(alpha, K), [estimate] anchor estimate after a plain "
                         "cross-entropy stage, or PATH.npy holding a [K,K] matrix C[clean, noisy]")
    f.DEFINE_integer("estimate_steps", 0, "--confusion_matrix estimate: steps of the plain cross-entropy stage (0: as many as the main run)")
    f.DEFINE_float("anchor_quantile", 0.97, "--confusion_matrix estimate: the quantile of estimate_confusion_anchor (1.0: the arg-max sample)")
    return f


def load_clean(FLAGS, n_classes, data_dir):
    """-> (train images [N,3072] u8 CHW, train labels, held-out images, held-out labels), labels uncorrupted."""
    if FLAGS.synthetic:
        n = FLAGS.synthetic_samples
        tx, ty = D.synthetic_cifar(n, 1234, FLAGS.synthetic_kind, n_classes)
        vx, vy = D.synthetic_cifar(max(n // 5, 1000), 1235, FLAGS.synthetic_kind, n_classes)
    elif FLAGS.dataset == "cifar100":
        tx, ty = D.unpickle100(os.path.join(data_dir, 'train'), FLAGS.coarse_labels)
        vx, vy = D.unpickle100(os.path.join(data_dir, 'test'), FLAGS.coarse_labels)
    else:
        parts = [D.unpickle(os.path.join(data_dir, 'data_batch_%d' % i)) for i in range(1, 6)]
        tx, ty = np.concatenate([p[0] for p in parts], axis=0), np.concatenate([p[1] for p in parts], axis=0)
        vx, vy = D.unpickle(os.path.join(data_dir, 'test_batch'))
    return np.asarray(tx), np.asarray(ty), np.asarray(vx), np.asarray(vy)


def lr_at(step, total, lr):
    """lr, divided by 10 from 50 % of the run on and again from 75 %."""
    return lr * (0.01 if 4 * step >= 3 * total else 0.1 if 2 * step >= total else 1.0)


def check_noise_flags(FLAGS):
    """The label-noise flags against each other, before anything is loaded.  -> the matrix source: None, 'known', 'estimate' or a path."""
    V.check_alpha(FLAGS)
    src = V.check_loss(FLAGS, ('known', 'estimate'))
    if FLAGS.estimate_steps < 0:
        raise ValueError('flag estimate_steps = %r' % (FLAGS.estimate_steps,))
    if not 0.0 < FLAGS.anchor_quantile <= 1.0:
        raise ValueError('flag anchor_quantile = %r: (0, 1]' % (FLAGS.anchor_quantile,))
    return src


def _in_chunks(fn, images_chw_u8, *rest, chunk=10000):
    """fn(NHWC images, *rest) over the set ``chunk`` images at a time (a multiple of the evaluation batch): host memory stays small."""
    outs = []
    for lo in range(0, len(images_chw_u8), chunk):
        x = images_chw_u8[lo:lo + chunk].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
        outs.append(fn(x, *[r[lo:lo + chunk] for r in rest]))
    return outs


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    FLAGS = define_flags().parse(argv)
    V.check_outputs(FLAGS)
    source = check_noise_flags(FLAGS)
    n_classes, data_dir = dataset_setup(FLAGS)
    logging.basicConfig(filename=FLAGS.log_file, level=logging.INFO, format='%(asctime)s %(levelname)-8s %(message)s')
    logging.info('dataset = {} ({} classes)'.format(FLAGS.dataset, n_classes))
    tx, ty, vx, vy = load_clean(FLAGS, n_classes, data_dir)
    held = vx.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    ty, ty_clean = V.corrupt_labels(FLAGS, ty, n_classes)
    from .classifier import LabelClassifierTrainer
    B = FLAGS.batch_size
    per_epoch = max(len(ty) // B, 1)
    total = FLAGS.max_steps if FLAGS.max_steps > 0 else FLAGS.epochs * per_epoch
    no_flip = np.zeros((B, 3), np.int32) if FLAGS.no_augment else None

    def run(n_steps, confusion_matrix):
        """A trainer from the flags' initialisation, trained for n_steps on the schedule that spans them.  -> (trainer, held-out accuracy)"""
        t = LabelClassifierTrainer(n_classes, batch_size=B, momentum=FLAGS.momentum, weight_decay=FLAGS.weight_decay, nesterov=FLAGS.nesterov,
                                   pad=0 if FLAGS.no_augment else 4, seed=FLAGS.seed, f32_matmul_precision=FLAGS.f32_matmul_precision,
                                   device=int(os.environ.get("LOCAL_RANK", "0")), confusion_matrix=confusion_matrix)
        t.load_data(tx, ty)
        return t, V.train(t, n_steps, per_epoch, lambda step: lr_at(step, n_steps, FLAGS.lr), held, vy, shift_flip=no_flip)

    Cm = None
    if source == 'estimate':
        n_est = FLAGS.estimate_steps if FLAGS.estimate_steps > 0 else total
        logging.info('confusion matrix: {} steps of plain cross-entropy on the noisy labels, then the anchor estimate'.format(n_est))
        t, _ = run(n_est, None)
        probs = np.concatenate(_in_chunks(lambda x: t.evaluate(x, np.zeros(len(x), np.int64))[1], tx), axis=0)
        t.close()
        Cm = V.row_normalised(D.estimate_confusion_anchor(probs, FLAGS.anchor_quantile))
        logging.info('estimated confusion matrix (quantile {:g}): diagonal mean {:.4f}, min {:.4f}'.format(
            FLAGS.anchor_quantile, float(np.diag(Cm).mean()), float(np.diag(Cm).min())))
        if ty_clean is not None:
            logging.info('estimate against C_ALPHA({}): largest entry error {:.4f}'.format(
                FLAGS.alpha, float(np.abs(Cm - D.C_ALPHA(FLAGS.alpha, n_classes)).max())))
    elif source is not None:
        Cm = V.load_matrix(FLAGS, source, n_classes)
    if Cm is not None:
        logging.info('loss = forward, confusion matrix from {}'.format(source))
    t, acc = run(total, Cm)
    t.save_asset(FLAGS.out)
    logging.info('wrote {} ({} classes, held-out accuracy {})'.format(FLAGS.out, n_classes, acc))
    if FLAGS.recover_out is not None:
        parts = _in_chunks(t.recover_labels, tx, ty)
        y_rec, post = np.concatenate([p[0] for p in parts], axis=0), np.concatenate([p[1] for p in parts], axis=0)
        V.write_recovered(FLAGS.recover_out, y_rec, post, ty, ty_clean, Cm)
    t.close()
    return acc


if __name__ == '__main__':
    main()
