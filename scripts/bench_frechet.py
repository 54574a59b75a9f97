#!/usr/bin/env python3
"""Cost of the Frechet metric (--frechet_freq of train_cifar.py), one MI355X:

  * wall time of ONE evaluation of 10 000 generated samples -- generate (100 Generator calls of 100), frozen features + per-class
    moments on the device, one download, the host distances -- at K = 10 and at K = 100 (bf16 generator, fp32 classifier);
  * rcgan_class_moments_accum per call of 1000 rows x 64 features, K = 10 and K = 100 (HIP events around a train of calls);
  * the training iteration with the flag off: bench.py of this tree, and of a checkout of the parent commit when --parent-root DIR
    names one (built), the two alternating as child processes.

usage: python scripts/bench_frechet.py [--samples 10000] [--repeats 3] [--parent-root DIR] [--out FILE]   (default: profiles/frechet.json)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rcgan_amd  # noqa: E402,F401


def evaluation(K, samples, repeats, n_real=2000):
    from rcgan_amd import data as D
    from rcgan_amd import frechet as FR
    from rcgan_amd.cifar import Z_DIM, CifarRCGAN
    from rcgan_amd.train_cifar import gen_acc_label_lists
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=64, dtype="bf16", seed=0, n_classes=K)
    ev = FR.FrechetEvaluator(K)
    rx, ry = D.synthetic_cifar(n_real, 1234, "templates", K)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    real_s = time.perf_counter() - t0
    rs = np.random.RandomState(0)
    balanced = gen_acc_label_lists(K, balanced=True)
    calls = [balanced[j % len(balanced)] for j in range(samples // 100)]
    rows = []
    for rep in range(repeats + 1):                 # the first one warms up (code objects, scratch) and is dropped
        t0 = time.perf_counter()
        x = [m.sample(labels, rs.normal(size=(100, Z_DIM)).astype('float32')) for labels in calls]
        x = ((np.concatenate(x, axis=0) + 1.) * (255.99 / 2)).astype('int32').reshape((-1, 32, 32, 3))
        t1 = time.perf_counter()
        mom = ev.moments(x, np.concatenate(calls, axis=0))
        t2 = time.perf_counter()
        r = FR.evaluate(ev.real, mom)
        t3 = time.perf_counter()
        if rep:
            rows.append(dict(generate_s=t1 - t0, features_moments_s=t2 - t1, host_distance_s=t3 - t2, total_s=t3 - t0))
    out = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    out.update(samples=len(x), real_images=n_real, real_statistics_s=real_s, classes_used=r["classes_used"], all_total_s=[r["total_s"] for r in rows])
    ev.close()
    m.ctx.close()
    return out


def kernel(K, calls=200, n=1000, d=64):
    import ctypes as C
    from rcgan_amd.runtime import Context
    ctx = Context(0, "f32", arena_bytes=1 << 26, ws_bytes=1 << 20)
    rs = np.random.RandomState(1)
    feat = ctx.upload(rs.randn(n, d).astype(np.float32))
    labels = ctx.upload(rs.randint(K, size=n))
    state = torch.zeros(ctx.lib.rcgan_class_moments_bytes(d, K) // 8, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    go = lambda: ctx.check(ctx.lib.rcgan_class_moments_accum(ctx.h, n, d, K, C.c_void_p(feat.ptr), C.c_void_p(labels.ptr), C.c_void_p(state.data_ptr())))
    for _ in range(10):
        go()
    ctx.sync()
    us = []
    for _ in range(5):
        ctx.event_record(0)
        for _ in range(calls):
            go()
        ctx.event_record(1)
        ctx.sync()
        us.append(ctx.event_elapsed_ms(0, 1) * 1e3 / calls)
    ctx.close()
    return dict(rows=n, d=d, us_per_call_median=statistics.median(us), min=min(us), max=max(us))


def bench_ms(root, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--no-cpu-baseline"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, check=True)
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    return float(res["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    out = {"kernel_source_hash": L.source_hash(), "generator_dtype": "bf16", "classifier_dtype": "f32"}
    for K in (10, 100):
        out["evaluation_K%d" % K] = evaluation(K, a.samples, a.repeats)
        out["moments_kernel_K%d" % K] = kernel(K)
    roots = {"this_tree": ROOT}
    if a.parent_root:
        roots["parent_commit"] = os.path.abspath(a.parent_root)
    ms = {name: [] for name in roots}
    for _ in range(a.bench_repeats):
        for name, root in roots.items():             # alternate the trees
            ms[name].append(bench_ms(root, a.bench_steps, 10))
    out["training_iteration_flag_off"] = {name: dict(ms_per_iter_median=statistics.median(v), all=v) for name, v in ms.items()}
    if not a.parent_root:
        out["training_iteration_flag_off"]["parent_commit"] = "not measured (no --parent-root)"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
