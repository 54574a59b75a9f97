#!/bin/bash
# Sliced Wasserstein distance on Laplacian-pyramid patches (how far the distribution of generated class-c IMAGES is from the
# distribution of real class-c images, per pyramid level: fine = texture and sharpness, middle = shapes, coarse = layout and colour),
# pooled and per class, beside its floor (two disjoint runs of the reference set at the same counts), between two sample dumps, one
# MI355X:
#   ./run_swd.sh --real real.npz --generated samples.npz  [--n_classes 10] [--directions 128]
# Each .npz holds `images` ([n,32,32,3], [n,3072] channel-major rows, [n,28,28,1] or [n,784] for MNIST dumps; raw pixels 0..255) and
# `labels` [n].  Prints one JSON line.  Needs no classifier and no weights.
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.swd "$@"
