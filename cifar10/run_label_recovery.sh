#!/bin/bash
# Train the label classifier (pre-activation ResNet-32, K classes) on NOISY training labels with the forward-corrected loss
# -log((softmax(z) . C)[label]) (Patrini et al. 2017), one MI355X, and recover the training labels.  Writes the weight asset -- a drop-in for
#   ./run_rcgan_cifar100.sh --label_classifier label_recovery/label_classifier.npz  -- and label_recovery/recovered_labels.npz (y_noisy,
# y_recover, posterior, confusion_matrix; recovery_accuracy and noisy_agreement when --alpha corrupted labels whose clean version is known).
# Default: CIFAR-100 fine labels from ../data/cifar100/cifar-100-python, corrupted once at --alpha 0.6, the known one-coin matrix.
#   --confusion_matrix estimate [--estimate_steps N --anchor_quantile 0.97]   the matrix from a plain cross-entropy stage (anchor estimate)
#   --confusion_matrix C.npy --alpha 1.0                                       labels that arrive noisy, the [K,K] matrix an RCGAN-U run learned
#   --coarse_labels: 20 classes; --dataset cifar: CIFAR-10 from ../data/cifar10.  Later flags override the defaults below.
out=label_recovery
mkdir -p "$out"
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.train_classifier --dataset cifar100 --alpha 0.6 --loss forward \
  --confusion_matrix known --log_file "$out/train_log.txt" --out "$out/label_classifier.npz" --recover_out "$out/recovered_labels.npz" "$@"
