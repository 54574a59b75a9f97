"""Train the MNIST generated-label-accuracy classifier (``mnist/run_label_classifier.sh``) and write the weight asset that
``train_mnist.py --label_classifier PATH`` scores generated samples with.

The reference scores with a frozen graph (mnist/mnist_dcnn/graph_optimized.pb) that the checkout does not hold; this trains the same
kind of network -- the "deep MNIST" convnet, mnist_classifier.py -- on the engine.  It trains on the CLEAN training labels: a
classifier trained on the corrupted ones would measure the label noise, not the generator.  The 10000 test images of
<data_dir>/mnist (a separate draw with --synthetic) are held out and scored after every epoch.

With only NOISY labels and a confusion matrix C: ``--loss forward`` trains on them with the forward-corrected loss
-log((softmax(z) . C)[label]) (Patrini et al. 2017), so the asset is still a drop-in for ``--label_classifier``; ``--recover_out`` then
writes the recovered training labels.  The matrix is ``known`` (the one-coin matrix of ``--alpha``) or a ``.npy`` file.  ``--alpha``
below 1 corrupts the training labels once; the clean ones are then kept for reporting only.

The label-noise flags and their checks, the corruption, matrix loading, the training loop and the writer of ``--recover_out`` are
``label_driver``'s, shared with ``train_classifier.py``.
"""
import logging
import os
import sys

import numpy as np

from . import data_mnist as DM
from . import label_driver as V
from .host import Flags

N_CLASSES = DM.Y_DIM


def define_flags():
    f = Flags()
    f.DEFINE_string("data_dir", "../data/", "Root directory of dataset: <data_dir>/mnist holds the four IDX files")
    f.DEFINE_boolean("synthetic", False, "train on the synthetic stand-in digits instead of the files under --data_dir")
    f.DEFINE_string("synthetic_kind", 'uniform', "with --synthetic: [uniform] label-free noise digits, [templates] class-pattern digits")
    f.DEFINE_integer("synthetic_samples", 60000, "with --synthetic: size of the training set (the held-out set is a sixth of it, at least 1000)")
    f.DEFINE_integer("epochs", 20, "passes over the training set")
    f.DEFINE_integer("max_steps", 0, "if > 0: stop after this many steps")
    f.DEFINE_integer("batch_size", 128, "batch size")
    f.DEFINE_float("lr", 1e-4, "Adam learning rate (constant)")
    f.DEFINE_float("keep_prob", 0.5, "dropout keep probability in front of the last dense layer, (0, 1]")
    f.DEFINE_integer("seed", 0, "seed of the initialisation, of the batch order and of the dropout stream")
    V.define_noise_flags(f, "10", "with --loss forward: [known] C_ALPHA(alpha, 10), or PATH.npy holding a [10,10] matrix C[clean, noisy]")
    return f


def check_flags(FLAGS):
    """The flags against each other, before anything is loaded.  -> the matrix source: None, 'known' or a path."""
    V.check_outputs(FLAGS)
    V.check_alpha(FLAGS)
    if not 0.0 < FLAGS.keep_prob <= 1.0:
        raise ValueError('flag keep_prob = %r: (0, 1]' % (FLAGS.keep_prob,))
    if FLAGS.batch_size < 1 or FLAGS.epochs < 0 or FLAGS.max_steps < 0:
        raise ValueError('flags batch_size = %r, epochs = %r, max_steps = %r' % (FLAGS.batch_size, FLAGS.epochs, FLAGS.max_steps))
    if FLAGS.loss == 'forward' and FLAGS.confusion_matrix == 'estimate':
        raise ValueError('--confusion_matrix estimate is not implemented for the MNIST classifier: known or PATH.npy')
    return V.check_loss(FLAGS, ('known',))


def load_clean(FLAGS):
    """-> (train images [N,28,28,1] float32 in [0, 1], train labels, held-out images, held-out labels), labels uncorrupted."""
    if FLAGS.synthetic:
        n = FLAGS.synthetic_samples
        tx, ty = DM.synthetic(n, 1234, FLAGS.synthetic_kind)
        vx, vy = DM.synthetic(max(n // 6, 1000), 1235, FLAGS.synthetic_kind)
    else:
        X, y = DM.read_idx(os.path.join(FLAGS.data_dir, "mnist"))           # train (60000) then t10k (10000), file order
        tx, ty, vx, vy = X[:60000], y[:60000], X[60000:], y[60000:]
    # the scaling data_mnist.corrupt / load_mnist hand to the GAN (and the sampler's output range): [0, 1]
    scale = lambda a: (np.asarray(a, np.float64) / 255.).astype(np.float32)
    return scale(tx), np.asarray(ty), scale(vx), np.asarray(vy)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    FLAGS = define_flags().parse(argv)
    source = check_flags(FLAGS)
    logging.basicConfig(filename=FLAGS.log_file, level=logging.INFO, format='%(asctime)s %(levelname)-8s %(message)s')
    logging.info('dataset = mnist ({} classes)'.format(N_CLASSES))
    tx, ty, vx, vy = load_clean(FLAGS)
    if tx.min() < 0.0 or tx.max() > 1.0:
        raise ValueError('images outside [0, 1] after scaling: [%g, %g]' % (tx.min(), tx.max()))
    ty, ty_clean = V.corrupt_labels(FLAGS, ty, N_CLASSES)
    Cm = None if source is None else V.load_matrix(FLAGS, source, N_CLASSES)
    if Cm is not None:
        logging.info('loss = forward, confusion matrix from {}'.format(source))
    from .mnist_classifier import MnistClassifierTrainer
    B = FLAGS.batch_size
    per_epoch = max(len(ty) // B, 1)
    total = FLAGS.max_steps if FLAGS.max_steps > 0 else FLAGS.epochs * per_epoch
    t = MnistClassifierTrainer(N_CLASSES, batch_size=B, keep_prob=FLAGS.keep_prob, seed=FLAGS.seed,
                               device=int(os.environ.get("LOCAL_RANK", "0")), confusion_matrix=Cm)
    t.load_data(tx, ty)
    acc = V.train(t, total, per_epoch, lambda step: FLAGS.lr, vx, vy)
    t.save_asset(FLAGS.out)
    logging.info('wrote {} ({} classes, held-out accuracy {})'.format(FLAGS.out, N_CLASSES, acc))
    if FLAGS.recover_out is not None:
        y_rec, post = t.recover_labels(tx, ty)
        V.write_recovered(FLAGS.recover_out, y_rec, post, ty, ty_clean, Cm)
    t.close()
    return acc


if __name__ == '__main__':
    main()
