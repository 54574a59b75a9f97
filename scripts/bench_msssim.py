#!/usr/bin/env python3
"""Cost of the intra-class MS-SSIM (--msssim_freq of train_cifar.py) and what it separates, one MI355X:

  * rcgan_msssim_pairs per call (HIP events around a train of calls, after a warm-up) at the default size -- 10 000 images,
    10 classes x 1000 pairs + 1000 pooled pairs -- for 32x32x3 and 28x28x1 images;
  * wall time of ONE MsssimEvaluator.evaluate at that size, split into the host's preparation (uint8 layout, the pair draw), the
    upload, the launch (to the end of the kernel), the download and the host arithmetic; each part ends in a synchronisation;
  * the float64 restatement (tests/msssim_ref.py) on the host for the first ``--ref-pairs`` of the same pairs, scaled up to all of
    them, and the kernel's largest error against it on those pairs;
  * what the number separates on template images (2000 per set, 200 pairs per class): a second draw of the real distribution, a
    collapsed set (one image per class plus noise of sigma 2) and a class-mixed set (the second draw with shuffled labels);
  * the training iteration with the flag off: bench.py of this tree, and of a built checkout of the parent commit when
    --parent-root DIR names one, the two alternating as child processes.

usage: python scripts/bench_msssim.py [--samples 10000] [--repeats 3] [--ref-pairs 50] [--parent-root DIR] [--out FILE]
(default: profiles/msssim.json)
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


def templates(seed, n, classes=K):
    from rcgan_amd import data as DT
    rs = np.random.RandomState(seed)
    labels = np.sort(np.arange(n) % classes)
    return DT.template_images(rs, labels).astype(np.uint8), labels            # [n,3072] CHW rows


def kernel(ctx, images, labels, pairs):
    from rcgan_amd import msssim as MS
    x = MS.as_uint8_nhwc(images)
    cp = MS.class_pairs(labels, K, pairs, MS.SEED)
    dx, dp = MS.upload(ctx, x, cp["pairs"])
    t = timed_calls(ctx, lambda: MS.msssim_pairs(ctx, dx, dp))
    t.update(images=len(x), shape=list(x.shape[1:]), pairs=len(cp["pairs"]), pairs_per_s=len(cp["pairs"]) / (t["ms_per_call_median"] * 1e-3))
    return t


def evaluation(samples, pairs, repeats, ref_pairs):
    from rcgan_amd import msssim as MS
    from tests import msssim_ref as MR
    rx, ry = templates(1234, samples)
    gx, gy = templates(1235, samples)
    ev = MS.MsssimEvaluator(K, pairs=pairs)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    real_s = time.perf_counter() - t0
    rows = []
    for rep in range(repeats + 1):                 # the first one warms up (code object, allocator) and is dropped
        ev.ctx.sync()
        t0 = time.perf_counter()
        r = ev.evaluate(gx, gy)
        t1 = time.perf_counter()
        x = MS.as_uint8_nhwc(gx)
        cp = MS.class_pairs(gy, K, pairs, ev.seed)
        t2 = time.perf_counter()
        dx, dp = MS.upload(ev.ctx, x, cp["pairs"])
        ev.ctx.sync()
        t3 = time.perf_counter()
        out = MS.msssim_pairs(ev.ctx, dx, dp)
        ev.ctx.sync()
        t4 = time.perf_counter()
        sc = MS.download(ev.ctx, out)
        t5 = time.perf_counter()
        MS.summarise(sc.astype(np.float64), cp, ev.real)
        t6 = time.perf_counter()
        if rep:
            rows.append(dict(evaluate_s=t1 - t0, host_prepare_s=t2 - t1, upload_s=t3 - t2, launch_s=t4 - t3, download_s=t5 - t4, host_arithmetic_s=t6 - t5))
    res = {k: statistics.median(r_[k] for r_ in rows) for k in rows[0]}
    t0 = time.perf_counter()
    want = MR.scales(x, cp["pairs"][:ref_pairs])
    ref_s = time.perf_counter() - t0
    res.update(samples=len(gx), real_images=len(rx), pairs_per_class=pairs, pairs_in_all=len(cp["pairs"]), prepare_real_s=real_s, all=rows,
               float64_restatement=dict(pairs=int(ref_pairs), seconds=ref_s, scaled_to_all_pairs_s=ref_s * len(cp["pairs"]) / ref_pairs),
               largest_error_against_float64=float(np.abs(sc[:ref_pairs] - want).max()), derived_bound=1e-4,
               result={k: r[k] for k in ("msssim", "intra_class_msssim", "intra_class_msssim_se", "intra_class_msssim_real", "classes_above_real",
                                         "classes_compared")})
    ev.close()
    return res


def separation(n=2000, pairs=200):
    from rcgan_amd import msssim as MS
    ev = MS.MsssimEvaluator(K, pairs=pairs)
    rx, ry = templates(22, n)
    ev.prepare_real(rx, ry)
    xb, lb = templates(23, n)
    rs = np.random.RandomState(25)
    one, _ = templates(24, K)
    collapsed = np.clip(one[lb].astype(np.float64) + 2.0 * rs.randn(n, 3072), 0, 255)
    sets = dict(independent_draw=(xb, lb), collapsed=(collapsed, lb), labels_shuffled=(xb, rs.permutation(lb)))
    out = dict(images_per_set=n, pairs_per_class=pairs)
    for name, (x, labels) in sets.items():
        r = ev.evaluate(x, labels)
        out[name] = {k: r[k] for k in ("msssim", "intra_class_msssim", "intra_class_msssim_se", "intra_class_msssim_real", "classes_above_real",
                                       "classes_compared")}
        out[name]["per_class"] = [None if np.isnan(v) else float(v) for v in r["per_class"]]
    out["real_per_class"] = [None if np.isnan(v) else float(v) for v in ev.real["per_class"]]
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-pairs", type=int, default=50)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash()}
    ctx = Context(0, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
    images, labels = templates(1, a.samples)
    out["kernel_32x32x3"] = kernel(ctx, images, labels, a.pairs)
    out["kernel_28x28x1"] = kernel(ctx, images.reshape(-1, 3, 32, 32)[:, 0, 2:30, 2:30], labels, a.pairs)
    ctx.close()
    print("kernel timed", file=sys.stderr, flush=True)
    out["evaluation"] = evaluation(a.samples, a.pairs, a.repeats, a.ref_pairs)
    print("evaluation timed", file=sys.stderr, flush=True)
    out["separation"] = separation()
    print("separation measured", file=sys.stderr, flush=True)
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
