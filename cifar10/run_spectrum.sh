#!/bin/bash
# Radial power-spectrum distance (do the generated class-c IMAGES carry their energy at the same spatial frequencies as the real
# class-c images: log-spectral distance, high-frequency, axis-Nyquist and checkerboard energy in dB), pooled and per class, beside its
# floor (two disjoint runs of the reference set at the same counts), between two sample dumps, one MI355X:
#   ./run_spectrum.sh --real real.npz --generated samples.npz  [--n_classes 10]
# Each .npz holds `images` ([n,32,32,3], [n,3072] channel-major rows, [n,28,28,1] or [n,784] for MNIST dumps; raw pixels 0..255) and
# `labels` [n].  Prints one JSON line.  Needs no classifier and no weights.
root="$(cd "$(dirname "$0")/.." && pwd)"
PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}" python -m rcgan_amd.spectrum "$@"
