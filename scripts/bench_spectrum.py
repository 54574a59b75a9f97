#!/usr/bin/env python3
"""Cost of the radial power-spectrum distance (--spectrum_freq of train_cifar.py) and what it separates, one MI355X:

  * the kernel of csrc/spectrum.hip (HIP events around a train of calls, after a warm-up) on 10 000 images of 32x32x3 and of
    28x28x1 already on the device, the upload of those images alone, and the segment sums (rcgan_class_moments_accum on the
    [n, c B] rows);
  * wall time of ONE SpectrumEvaluator.evaluate at that size (10 000 generated against 20 000 real images), the first one (which
    also takes the floor) and the later ones;
  * the largest error of the kernel as a fraction of the bound its header derives, per image family of tests/spectrum_ref.py;
  * the table of orderings (80 real and 40 generated images per class, 4 classes, 32x32x3): a fresh draw, the draw blurred, with a
    +-6 checkerboard, with +-6 column stripes -- on the device, beside the float64 restatement and the largest relative difference
    between the float64 restatement and its fp32 restatement (the evaluator test's tolerance is ten times that);
  * the training iteration with the flag off: bench.py of this tree, and of a built checkout of the parent commit when
    --parent-root DIR names one, the two alternating as child processes.

usage: python scripts/bench_spectrum.py [--samples 10000] [--repeats 3] [--parent-root DIR] [--out FILE]
(default: profiles/spectrum.json)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import rcgan_amd  # noqa: E402,F401
from bench_manifold import bench_ms, timed_calls  # noqa: E402

K = 10
NAMES = ("spectral_distance", "high_frequency_db", "nyquist_db", "checkerboard_db")


def calls(ctx, n, N, c):
    import torch
    from rcgan_amd import spectrum as SP
    x = np.random.RandomState(n + N).randint(0, 256, size=(n, N, N, c)).astype(np.uint8)
    labels = (np.arange(n) % K).astype(np.int32)
    with torch.cuda.stream(ctx.stream):
        host = torch.from_numpy(x).pin_memory()
        dx = host.to(ctx.device)
        out = SP.radial_spectrum(ctx, dx)
        rows = out.reshape(n, -1)
    res = dict(images=n, side=N, channels=c, rings=out.shape[2], megabytes=x.nbytes / 1e6)
    res["radial_spectrum"] = timed_calls(ctx, lambda: SP.radial_spectrum(ctx, dx, out=out))
    with torch.cuda.stream(ctx.stream):
        res["upload_pinned"] = timed_calls(ctx, lambda: dx.copy_(host, non_blocking=True))
    res["class_sums_with_download"] = timed_calls(ctx, lambda: SP.class_sums(ctx, rows, labels, K), window_ms=100.0)
    return res


def evaluation(samples, repeats):
    from rcgan_amd import spectrum as SP
    from tests import spectrum_ref as SR
    rs = np.random.RandomState(1)
    ry, gy = np.arange(2 * samples) % K, np.arange(samples) % K
    draw = lambda n: np.concatenate([SR.quantise(SR.blurred_noise(rs, min(1000, n - i), 32, 3)) for i in range(0, n, 1000)])
    rx, gx = draw(2 * samples), draw(samples)
    ev = SP.SpectrumEvaluator(K)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    ev.ctx.sync()
    real_s = time.perf_counter() - t0
    times = []
    for rep in range(repeats + 1):                 # the first one also takes the floor (and warms up code objects and the allocator)
        ev.ctx.sync()
        t0 = time.perf_counter()
        r = ev.evaluate(gx, gy)
        times.append(time.perf_counter() - t0)
    ev.close()
    return dict(samples=samples, real_images=len(rx), prepare_real_s=real_s, first_evaluate_with_floor_s=times[0],
                evaluate_s=statistics.median(times[1:]), all=times, result=SP.json_ready(r))


def error_over_bound(ctx):
    import torch
    from rcgan_amd import spectrum as SP
    from tests import spectrum_ref as SR
    out = {}
    for N, c in ((9, 3), (28, 1), (32, 3)):
        for name, x in SR.families(N, c, 67).items():
            with torch.cuda.stream(ctx.stream):
                dx = torch.from_numpy(x).to(ctx.device)
            got = SP.download(ctx, SP.radial_spectrum(ctx, dx)).astype(np.float64)
            err, bound = np.abs(got - SR.spectrum(x)), SR.bound(x)
            out["%dx%dx%d %s" % (N, N, c, name)] = float((err / bound).max()) if name != "constant_128" else float(err.max())
    out["largest"] = max(out.values())
    return out


def orderings():
    from rcgan_amd import spectrum as SP
    from tests import spectrum_ref as SR
    out = {}
    for classes, per_class, N, c in ((4, 40, 32, 3), (2, 30, 28, 1)):
        w = SR.world(classes, per_class, N, c)
        ev = SP.SpectrumEvaluator(classes)
        ev.prepare_real(w["real"], w["real_labels"])
        table = dict(classes=classes, generated_per_class=per_class, real_per_class=2 * per_class, side=N, channels=c)
        worst = 0.0
        for name in ("fresh", "blurred", "checker", "striped"):
            r = ev.evaluate(w[name], w["labels"])
            ref = SR.evaluate(w["real"], w["real_labels"], w[name], w["labels"], classes)
            f32 = SR.evaluate(w["real"], w["real_labels"], w[name], w["labels"], classes, spectrum_fn=SR.spectrum_f32)
            worst = max(worst, SR.relative_difference(ref, f32))
            table[name] = dict(device={n: r[n] for n in NAMES}, float64={n: ref[n] for n in NAMES},
                               intra_class_spectral_distance=r["intra_class_spectral_distance"],
                               device_against_float64_relative=SR.relative_difference(ref, r))
            table["floor"] = dict(spectral_distance=r["floor_spectral_distance"], intra_class_spectral_distance=r["floor_intra_class_spectral_distance"])
        table["float64_against_fp32_restatement_relative"] = worst
        table["evaluator_test_tolerance"] = 10.0 * worst
        ev.close()
        out["%dx%dx%d" % (N, N, c)] = table
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash()}
    ctx = Context(0, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
    out["calls_32x32x3"] = calls(ctx, a.samples, 32, 3)
    out["calls_28x28x1"] = calls(ctx, a.samples, 28, 1)
    print("calls timed", file=sys.stderr, flush=True)
    out["error_over_bound"] = error_over_bound(ctx)
    ctx.close()
    print("errors measured", file=sys.stderr, flush=True)
    out["evaluation"] = evaluation(a.samples, a.repeats)
    print("evaluation timed", file=sys.stderr, flush=True)
    out["orderings"] = orderings()
    print("orderings measured", file=sys.stderr, flush=True)
    roots = {"this_tree": ROOT}
    if a.parent_root:
        roots["parent_commit"] = os.path.abspath(a.parent_root)
    ms = {name: [] for name in roots}
    for _ in range(a.bench_repeats):
        for name, root in roots.items():             # alternate the trees
            ms[name].append(bench_ms(root, a.bench_steps, 10))
            print("bench.py of %s: %.3f ms" % (name, ms[name][-1]), file=sys.stderr, flush=True)
    out["training_iteration_flag_off"] = {name: dict(ms_per_iter_median=statistics.median(v), all=v) for name, v in ms.items()}
    if not a.parent_root:
        out["training_iteration_flag_off"]["parent_commit"] = "not measured (no --parent-root)"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
