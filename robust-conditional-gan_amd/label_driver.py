"""What the two label-classifier command lines share (train_classifier.py, train_mnist_classifier.py): the label-noise flags and their
checks, the one-time corruption of the training labels, the confusion matrix from ``known`` or a ``.npy`` file, the train / evaluate /
log loop and the writer of ``--recover_out``.  Each script keeps its own flags, its data, its learning-rate rule and its trainer.
"""
import logging
import time

import numpy as np

from . import data as D


def define_noise_flags(f, k, matrix_help):
    """The flags of both command lines; k: the class count as the help texts name it."""
    f.DEFINE_float("alpha", 1.0, "< 1: corrupt the training labels once through the one-coin matrix C_ALPHA(alpha, %s); 1.0: clean labels" % k)
    f.DEFINE_integer("label_seed", 0, "seed of the label corruption")
    f.DEFINE_string("loss", 'ce', "[ce] sparse softmax cross-entropy, [forward] forward-corrected for noisy labels (needs --confusion_matrix)")
    f.DEFINE_string("confusion_matrix", None, matrix_help)
    f.DEFINE_string("recover_out", None, "with --loss forward: where the recovered training labels (.npz) are written")
    f.DEFINE_string("out", None, "where the weight asset (.npz) is written")
    f.DEFINE_string("log_file", None, "logging file")


def check_outputs(FLAGS):
    if FLAGS.log_file is None:
        raise ValueError('flag log_file is required')
    if FLAGS.out is None:
        raise ValueError('flag out is required')


def check_alpha(FLAGS):
    if not 0.0 < FLAGS.alpha <= 1.0:
        raise ValueError('flag alpha = %r: (0, 1]' % (FLAGS.alpha,))


def check_loss(FLAGS, sources):
    """--loss, --confusion_matrix and --recover_out against each other.  sources: the matrix sources by name that the command line
    knows beside PATH.npy.  -> the matrix source: None, one of ``sources`` or a path."""
    if FLAGS.loss not in ('ce', 'forward'):
        raise ValueError('flag loss = %r: ce or forward' % (FLAGS.loss,))
    src = FLAGS.confusion_matrix
    if FLAGS.loss == 'forward' and src is None:
        raise ValueError('--loss forward needs --confusion_matrix [%s, PATH.npy]' % ', '.join(sources))
    if FLAGS.loss == 'ce' and src is not None:
        raise ValueError('--confusion_matrix is read by --loss forward only')
    if FLAGS.loss == 'ce' and FLAGS.recover_out is not None:
        raise ValueError('--recover_out needs --loss forward')
    if src is not None and src not in sources and not src.endswith('.npy'):
        raise ValueError('flag confusion_matrix = %r: %s or PATH.npy' % (src, ', '.join(sources)))
    return src


def corrupt_labels(FLAGS, ty, n_classes):
    """-> (training labels, clean labels or None).  --alpha below 1: the training labels arrive noisy -- corrupted once, the clean ones
    kept for reporting only (the held-out labels stay clean)."""
    if not FLAGS.alpha < 1.0:
        return ty, None
    noisy = D.noisy_labels(ty, D.C_ALPHA(FLAGS.alpha, n_classes), np.random.RandomState(FLAGS.label_seed))
    logging.info('alpha = {}: training labels corrupted (label_seed {}), {:.4f} of them still agree with the clean ones'.format(
        FLAGS.alpha, FLAGS.label_seed, float((noisy == ty).mean())))
    return noisy, ty


def row_normalised(C):
    """A matrix that was stored or computed in float32: rows brought to sum 1 in float64 (the trainer asks for 1e-6)."""
    C = np.asarray(C, np.float64)
    return C / C.sum(axis=1, keepdims=True)


def load_matrix(FLAGS, source, n_classes):
    """The confusion matrix of source ``known`` or PATH.npy."""
    if source == 'known':
        return D.C_ALPHA(FLAGS.alpha, n_classes)
    return D.check_confusion_matrix(row_normalised(np.load(source)), n_classes)


def train(t, n_steps, per_epoch, lr_of, held, held_labels, **step_args):
    """n_steps of t.step(lr_of(step), **step_args); after every epoch and after the last step the held-out set is scored and a line
    logged.  -> the last held-out accuracy (None without steps)."""
    t0 = time.time()
    acc = None
    for step in range(n_steps):
        t.step(lr_of(step), **step_args)
        if (step + 1) % per_epoch == 0 or step + 1 == n_steps:
            loss, batch_acc = t.losses()
            acc, _ = t.evaluate(held, held_labels)
            logging.info('epoch {} step {} lr {:g} loss {:.4f} batch accuracy {:.4f} held-out accuracy {:.4f} ({:.0f} s)'.format(
                (step + 1) // per_epoch, step + 1, lr_of(step), loss, batch_acc, acc, time.time() - t0))
    return acc


def write_recovered(path, y_rec, post, ty, ty_clean, Cm):
    """The --recover_out file, and what it says about the recovery in the log."""
    fields = dict(y_noisy=np.asarray(ty, np.int64), y_recover=y_rec.astype(np.int64), posterior=post, confusion_matrix=Cm)
    if ty_clean is not None:
        fields.update(recovery_accuracy=float((y_rec == ty_clean).mean()), noisy_agreement=float((ty == ty_clean).mean()))
        logging.info('label recovery accuracy {:.4f} (noisy labels agree with clean: {:.4f})'.format(
            fields['recovery_accuracy'], fields['noisy_agreement']))
    else:
        logging.info('label recovery: {:.4f} of the recovered labels differ from the given ones (no clean labels to score against)'.format(
            float((y_rec != ty).mean())))
    with open(path, 'wb') as f:
        np.savez(f, **fields)
    logging.info('wrote {}'.format(path))
