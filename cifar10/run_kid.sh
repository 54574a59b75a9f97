#!/bin/bash
# Kernel distance (the unbiased cubic-polynomial-kernel MMD^2 of the Kernel Inception Distance; pooled, per class, and mean +- std
# over subsets) between two sample dumps on the label classifier's 64-wide frozen-statistics feature, one MI355X:
#   ./run_kid.sh --real real.npz --generated samples.npz  [--n_classes 10] [--subset_size 1000]
#                [--label_classifier label_classifier/label_classifier.npz]
# Each .npz holds `images` ([n,32,32,3] or [n,3072] channel-major rows, raw pixels 0..255) and `labels` [n]; the first 1000 images
# of --real calibrate the features.  Prints one JSON line.  Not comparable with published Inception KID values.
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.kid "$@"
