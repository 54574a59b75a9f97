#!/bin/bash
# Train the MNIST generated-label-accuracy classifier (the "deep MNIST" convnet: two 5x5 convolutions with ReLU + 2x2 max pool, a
# 1024-wide dense layer, dropout, a 10-way dense layer) on the CLEAN training labels of ../data/mnist, one MI355X, and write the weight
# asset that  ./run_rcgan.sh --label_classifier label_classifier/mnist_label_classifier.npz  scores generated samples with.
# Without the data set:  ./run_label_classifier.sh --synthetic --synthetic_kind templates.  Extra flags pass through.
out=label_classifier
mkdir -p "$out"
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.train_mnist_classifier \
  --log_file "$out/train_log.txt" --out "$out/mnist_label_classifier.npz" "$@"
