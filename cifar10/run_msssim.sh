#!/bin/bash
# Intra-class MS-SSIM (the multi-scale structural similarity of random pairs of IMAGES of one class, class by class, beside the same
# number on the reference set: a class whose generated pairs are more alike than its real pairs has lost modes) between two sample
# dumps, one MI355X:
#   ./run_msssim.sh --real real.npz --generated samples.npz  [--n_classes 10] [--pairs 1000] [--seed N]
# Each .npz holds `images` ([n,32,32,3], [n,3072] channel-major rows, [n,28,28,1] or [n,784] for MNIST dumps; raw pixels 0..255) and
# `labels` [n].  Prints one JSON line.  Needs no classifier and no weights.
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.msssim "$@"
