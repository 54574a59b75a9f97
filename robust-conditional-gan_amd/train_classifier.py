"""Train the generated-label-accuracy classifier for a data set (``cifar10/run_label_classifier.sh``) and write the weight asset
that ``train_cifar.py --label_classifier PATH`` scores generated samples with.

Trains on the CLEAN training labels: a classifier trained on the corrupted ones would measure the label noise, not the generator.
The held-out set is scored under the evaluator's protocol (batches of 1000, every batch norm on the moments of its batch).
"""
import logging
import os
import sys
import time

import numpy as np

from . import data as D
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
    f.DEFINE_string("out", None, "where the weight asset (.npz) is written")
    f.DEFINE_string("log_file", None, "logging file")
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


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    FLAGS = define_flags().parse(argv)
    if FLAGS.log_file is None:
        raise ValueError('flag log_file is required')
    if FLAGS.out is None:
        raise ValueError('flag out is required')
    n_classes, data_dir = dataset_setup(FLAGS)
    logging.basicConfig(filename=FLAGS.log_file, level=logging.INFO, format='%(asctime)s %(levelname)-8s %(message)s')
    logging.info('dataset = {} ({} classes)'.format(FLAGS.dataset, n_classes))
    tx, ty, vx, vy = load_clean(FLAGS, n_classes, data_dir)
    held = vx.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    from .classifier import LabelClassifierTrainer
    B = FLAGS.batch_size
    t = LabelClassifierTrainer(n_classes, batch_size=B, momentum=FLAGS.momentum, weight_decay=FLAGS.weight_decay, nesterov=FLAGS.nesterov,
                               pad=0 if FLAGS.no_augment else 4, seed=FLAGS.seed, f32_matmul_precision=FLAGS.f32_matmul_precision,
                               device=int(os.environ.get("LOCAL_RANK", "0")))
    t.load_data(tx, ty)
    per_epoch = max(len(ty) // B, 1)
    total = FLAGS.max_steps if FLAGS.max_steps > 0 else FLAGS.epochs * per_epoch
    no_flip = np.zeros((B, 3), np.int32) if FLAGS.no_augment else None
    t0 = time.time()
    acc = None
    for step in range(total):
        t.step(lr_at(step, total, FLAGS.lr), shift_flip=no_flip)
        if (step + 1) % per_epoch == 0 or step + 1 == total:
            loss, batch_acc = t.losses()
            acc, _ = t.evaluate(held, vy)
            logging.info('epoch {} step {} lr {:g} loss {:.4f} batch accuracy {:.4f} held-out accuracy {:.4f} ({:.0f} s)'.format(
                (step + 1) // per_epoch, step + 1, lr_at(step, total, FLAGS.lr), loss, batch_acc, acc, time.time() - t0))
    t.save_asset(FLAGS.out)
    logging.info('wrote {} ({} classes, held-out accuracy {})'.format(FLAGS.out, n_classes, acc))
    t.close()
    return acc


if __name__ == '__main__':
    main()
