#!/bin/bash
# Train the generated-label-accuracy classifier (pre-activation ResNet-32, K classes) on the CLEAN training labels, one MI355X, and
# write the weight asset that  ./run_rcgan_cifar100.sh --label_classifier label_classifier/label_classifier.npz  scores generated
# samples with.  Default: CIFAR-100 fine labels from ../data/cifar100/cifar-100-python; --coarse_labels: 20 classes;
# --dataset cifar: CIFAR-10 from ../data/cifar10.
out=label_classifier
mkdir -p "$out"
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.train_classifier --dataset cifar100 \
  --log_file "$out/train_log.txt" --out "$out/label_classifier.npz" "$@"
