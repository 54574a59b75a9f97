#!/usr/bin/env python3
"""fp32 matmul precision "highest" (fp32 matrix cores) vs "high" (split-bf16 matrix cores) in ONE process, alternating the two:

  * the CIFAR fp32 iteration, B = 64 (bench.build_pool / bench.iteration, as scripts/step_times.py drives them)
  * the MNIST fp32 iteration, B = 256 (1 D + 2 G updates, as scripts/bench_mnist.py)
  * per-launch gather-GEMM convolutions on the scripts/bench_direct.py shapes (HIP events around each call)

usage:
  python scripts/bench_f32_precision.py [--out profiles/f32_precision.json] [--repeats 5]
      timing run: writes the JSON (ms / iteration, images/s, per-launch times, spread = min / max / stdev over the repeats)
  python scripts/bench_f32_precision.py --trace {cifar,mnist} {highest,high} [--iters N]
      N iterations of one configuration, nothing else: run it under rocprofv3 --kernel-trace --stats
  python scripts/bench_f32_precision.py --add-stats {cifar,mnist} {highest,high} KERNEL_STATS_CSV [--out ...]
      adds that trace's gather-GEMM rows (per iteration) to the JSON.  A split launch's share of peak is quoted against
      3 x the algorithmic FLOPs on the bf16 matrix peak (it issues three bf16 products per fp32 product)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import rcgan_amd  # noqa: E402,F401
from rcgan_amd import _lib as L  # noqa: E402

MODES = ("highest", "high")
PEAK_F32_TF, PEAK_BF16_TF = 157.3, 2500.0      # MI355X dense peaks (fp32 matrix = vector rate; bf16)
CIFAR_B, MNIST_B = 64, 256
DIRECT_SHAPES = [   # scripts/bench_direct.py: name, n, h, w, cin, cout, k, stride
    ("g_h2 deconv 7>14 138>128 (as conv 14>7 128>138)", MNIST_B, 14, 14, 128, 138, 5, 2),
    ("g_h3 deconv 14>28 138>1 (as conv 28>14 1>138)", MNIST_B, 28, 28, 1, 138, 5, 2),
    ("d_h0 conv 28>14 1>64", MNIST_B, 28, 28, 1, 64, 5, 2),
    ("d_h1 conv 14>7 64>64", MNIST_B, 14, 14, 64, 64, 5, 2),
    ("d_h2 conv 7>4 64>64", MNIST_B, 7, 7, 64, 64, 5, 2),
    ("d_h3 conv 4>2 64>64", MNIST_B, 4, 4, 64, 64, 5, 2),
]


def cifar_model(mode):
    from rcgan_amd.cifar import CifarRCGAN
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=CIFAR_B, dtype="f32", seed=0, device=0, f32_matmul_precision=mode)
    pool = bench.build_pool(m, 0, 0.6)
    state = dict(it=0, dc=[0])

    def run(n):
        for _ in range(n):
            bench.iteration(m, pool, state["it"], state["dc"])
            state["it"] += 1
    return m, run


def mnist_model(mode):
    from rcgan_amd.mnist import MnistRCGAN
    B = MNIST_B
    m = MnistRCGAN(algorithm="rcgan", alpha=0.3, batch_size=B, dtype="f32", disc_type="projection", estimate_confuse=False,
                   f32_matmul_precision=mode)
    rs = np.random.RandomState(0)
    eye = np.eye(10, dtype=np.float32)
    m.set_inputs(images=rs.rand(B, 28, 28, 1).astype(np.float32), z=rs.uniform(-1, 1, size=(B, 100)).astype(np.float32),
                 y_real=eye[rs.randint(10, size=B)], y_gen=eye[rs.randint(10, size=B)], y_fake=eye[rs.randint(10, size=B)],
                 y_real_weights=rs.randn(B, 10).astype(np.float32))

    def run(n):
        for _ in range(n):
            m.iteration()
    return m, run


def timed_ms(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), stdev=statistics.stdev(v) if len(v) > 1 else 0.0, samples=v)


def direct_launches(repeats, reps=20):
    """per-call time of the fp32 convolution forward / data gradient / filter gradient on the bench_direct shapes, both modes on
    one context, alternating"""
    from rcgan_amd.runtime import Context
    ctx = Context(0, "f32", arena_bytes=4 << 30, ws_bytes=1 << 30)
    lib, h = ctx.lib, ctx.h
    out = {}
    for name, n, hh, ww, cin, cout, k, s in DIRECT_SHAPES:
        ctx.new_step()
        oh, ow = (hh + s - 1) // s, (ww + s - 1) // s
        x, y = ctx.empty((n, hh, ww, cin)), ctx.empty((n, oh, ow, cout))
        dx = ctx.empty((n, hh, ww, cin))
        w, dw = ctx.empty((k, k, cin, cout), L.F32), ctx.empty((k, k, cin, cout), L.F32)
        for t in (x, y):
            ctx.check(lib.rcgan_rng_fill(h, t.size, t.dtype, 1, 0.0, 1.0, 7, None, C.c_void_p(t.ptr)))
        ctx.check(lib.rcgan_rng_fill(h, w.size, L.F32, 1, 0.0, 0.05, 9, None, C.c_void_p(w.ptr)))
        desc = L.ConvDesc(n, hh, ww, cin, cout, k, k, s, L.F32, 0)
        prep = ctx.arena.alloc(lib.rcgan_conv_prepared_bytes(C.byref(desc)))
        ctx.check(lib.rcgan_conv_prepare(h, C.byref(desc), C.c_void_p(w.ptr), None, C.c_void_p(prep)))
        flops = 2.0 * n * oh * ow * k * k * cin * cout
        calls = {
            "fwd": lambda: lib.rcgan_conv2d_fwd(h, C.byref(desc), C.c_void_p(x.ptr), C.c_void_p(prep), None, C.c_void_p(y.ptr)),
            "dgrad": lambda: lib.rcgan_conv2d_bwd_data(h, C.byref(desc), C.c_void_p(y.ptr), C.c_void_p(prep), None, C.c_void_p(dx.ptr),
                                                       C.c_void_p(ctx.ws_ptr), ctx.ws_bytes),
            "wgrad": lambda: lib.rcgan_conv2d_bwd_weight(h, C.byref(desc), C.c_void_p(x.ptr), C.c_void_p(y.ptr), C.c_void_p(dw.ptr), None,
                                                         0, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes),
        }
        row = {"gflop": flops / 1e9}
        for op, call in calls.items():
            us = {m: [] for m in MODES}
            for _ in range(repeats):
                for mode in MODES:
                    ctx.set_f32_matmul_precision(mode)
                    ctx.check(call())
                    ctx.check(call())
                    ctx.event_record(0)
                    for _ in range(reps):
                        ctx.check(call())
                    ctx.event_record(1)
                    us[mode].append(ctx.event_elapsed_ms(0, 1) * 1e3 / reps)
            row[op] = {m: spread(us[m]) for m in MODES}
            t_hx, t_hi = row[op]["highest"]["median"] * 1e-6, row[op]["high"]["median"] * 1e-6
            row[op]["tflops_algorithmic"] = {"highest": flops / t_hx / 1e12, "high": flops / t_hi / 1e12}
            # share of peak: highest against the fp32 matrix peak; high: 3 x the algorithmic FLOPs against the bf16 matrix peak
            row[op]["share_of_peak"] = {"highest (fp32 peak)": flops / t_hx / 1e12 / PEAK_F32_TF,
                                        "high (3 x algorithmic FLOPs on the bf16 peak)": 3 * flops / t_hi / 1e12 / PEAK_BF16_TF}
        out[name] = row
        print("%-50s" % name, "  ".join("%s %.1f -> %.1f us" % (op, row[op]["highest"]["median"], row[op]["high"]["median"])
                                       for op in calls), flush=True)
    ctx.set_f32_matmul_precision("highest")
    ctx.close()
    return out


def timing(args):
    from rcgan_amd.cifar import N_CRITIC
    res = dict(what="fp32 matmul precision highest vs high, one process, modes alternated", repeats=args.repeats)
    for model, make, iters, imgs in (("cifar", cifar_model, args.cifar_iters, CIFAR_B * N_CRITIC), ("mnist", mnist_model, args.mnist_iters, MNIST_B)):
        ms = {m: [] for m in MODES}
        built = {m: make(m) for m in MODES}
        for m in MODES:
            built[m][1](5)                              # warm-up: code objects, captures
        for _ in range(args.repeats):
            for m in MODES:
                ms[m].append(timed_ms(built[m][1], iters))
        for m in MODES:
            built[m][0].ctx.close()
        res[model] = dict(batch=CIFAR_B if model == "cifar" else MNIST_B, iterations_per_sample=iters, images_per_iteration=imgs,
                          ms_per_iteration={m: spread(ms[m]) for m in MODES},
                          images_per_s={m: imgs / statistics.median(ms[m]) * 1e3 for m in MODES},
                          speedup=statistics.median(ms["highest"]) / statistics.median(ms["high"]))
        print(model, {m: "%.3f ms (%.3f..%.3f)" % (statistics.median(ms[m]), min(ms[m]), max(ms[m])) for m in MODES}, flush=True)
    res["gather_gemm_launches"] = direct_launches(args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def trace(model, mode, iters):
    m, run = (cifar_model if model == "cifar" else mnist_model)(mode)
    run(iters)                  # no warm-up: every traced gather launch belongs to one of the `iters` iterations
    torch.cuda.synchronize()
    m.ctx.close()
    print("traced %d %s iterations (%s)" % (iters, model, mode))


def add_stats(model, mode, csv_path, iters, out):
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    gg = [r for r in rows if "gemm_gather_kernel" in r["Name"]]
    gg_ns = sum(float(r["TotalDurationNs"]) for r in gg)
    res = json.load(open(out))
    ent = res.setdefault(model, {}).setdefault("kernel_trace", {})
    ent[mode] = dict(iterations=iters, gpu_ms_per_iteration=total_ns / 1e6 / iters, gather_ms_per_iteration=gg_ns / 1e6 / iters,
                     gather_launches_per_iteration=sum(int(r["Calls"]) for r in gg) / iters,
                     gather_kernels=sorted(((r["Name"].split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6 / iters) for r in gg),
                                           key=lambda t: -t[2])[:12])
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(model, mode, "gather GEMM %.3f of %.3f ms GPU time per iteration" % (ent[mode]["gather_ms_per_iteration"], ent[mode]["gpu_ms_per_iteration"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/f32_precision.json")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cifar_iters", type=int, default=20)
    ap.add_argument("--mnist_iters", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trace", nargs=2, metavar=("MODEL", "MODE"))
    ap.add_argument("--add-stats", nargs=3, metavar=("MODEL", "MODE", "CSV"))
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace[0], args.trace[1], args.iters)
    if args.add_stats:
        return add_stats(args.add_stats[0], args.add_stats[1], args.add_stats[2], args.iters, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("bench_f32_precision.py measures the GPU: no HIP device visible")
    timing(args)


if __name__ == "__main__":
    main()
