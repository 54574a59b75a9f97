#!/bin/bash
# Nearest training images in pixel space (does the generator memorise?): copy rate, nearest-neighbour distance z and leave-one-out 1-NN
# accuracy of a sample dump against a training set, beside a held-out real set, one MI355X:
#   ./run_neighbours.sh --real train.npz --heldout test.npz --generated samples.npz  [--n_classes 10]
# Each .npz holds `images` ([n,32,32,3], [n,3072] channel-major rows, [n,28,28,1] or [n,784] for MNIST dumps; raw pixels 0..255) and
# `labels` [n].  Prints one JSON line.  Needs no classifier and no weights; distances are exact.
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.neighbours "$@"
