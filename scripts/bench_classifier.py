#!/usr/bin/env python3
"""Speed of the label classifier's training step (classifier.LabelClassifierTrainer, B = 128, fp32), recorded in
profiles/classifier_step.json -- the parent number of any later work on its kernels (its 16 / 32 / 64-channel convolutions run on
the generic 64 x 64 fp32 gather GEMM).

usage:
  python scripts/bench_classifier.py [--out profiles/classifier_step.json] [--classes 100] [--precision highest]
      timing run: HIP events around 50 replayed (captured) steps after 10 warm-up steps, three repetitions, median; and, in the same
      process, rcgan_shortcut_a_fwd / _bwd beside rcgan_meanpool2 + rcgan_pad_channels on the two shapes of the network
  python scripts/bench_classifier.py --trace [--iters 30]
      warm-up + N steps and nothing else: run it under  rocprofv3 --kernel-trace --stats -d DIR -o kt -- python scripts/bench_classifier.py --trace
      (a run of its own), then  python scripts/prof_summary.py DIR/.../kt_results.db 40 --csv KERNEL_STATS_CSV  (rocprofv3 writes a rocpd
      database; a kernel_stats.csv it wrote itself has the same Name / TotalDurationNs columns)
  python scripts/bench_classifier.py --add-stats KERNEL_STATS_CSV [--out ...]
      adds the share of the traced GPU time spent in the gather GEMM (and the ten heaviest kernels) to the JSON
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

B, WARMUP, STEPS, REPS = 128, 10, 50, 3
GEMM = "gemm_gather_kernel"


def trainer(classes, precision):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from rcgan_amd.classifier import LabelClassifierTrainer
    t = LabelClassifierTrainer(classes, batch_size=B, seed=0, f32_matmul_precision=precision)
    t.load_data(*D.synthetic_cifar(12800, 1234, "uniform", classes))
    return t


def time_steps(t):
    for _ in range(WARMUP):
        t.step(0.1)
    ms = []
    for _ in range(REPS):
        t.ctx.event_record(0)
        for _ in range(STEPS):
            t.step(0.1)
        t.ctx.event_record(1)
        t.ctx.sync()
        ms.append(t.ctx.event_elapsed_ms(0, 1) / STEPS)
    return ms


def time_shortcut(ctx, n, h, w, c, iters=200):
    """us per call: shortcut_a forward / backward, and the two-launch forms they replace, same process, same buffers."""
    from rcgan_amd import _lib as L
    x = ctx.persistent((n, h, w, c), L.F32, fill=0.5)
    mid = ctx.persistent((n, h // 2, w // 2, c), L.F32, fill=0.0)
    y = ctx.persistent((n, h // 2, w // 2, 2 * c), L.F32, fill=0.25)
    dx = ctx.persistent((n, h, w, c), L.F32, fill=0.0)
    p = lambda t: C.c_void_p(t.ptr)
    lib, hd = ctx.lib, ctx.h
    rows = n * (h // 2) * (w // 2)
    forms = {
        "shortcut_a_fwd": lambda: lib.rcgan_shortcut_a_fwd(hd, n, h, w, c, L.F32, p(x), p(y)),
        "meanpool2_fwd+pad_channels": lambda: (lib.rcgan_meanpool2_fwd(hd, n, h, w, c, L.F32, p(x), p(mid)),
                                               lib.rcgan_pad_channels(hd, rows, c, c // 2, c // 2, L.F32, p(mid), p(y))),
        "shortcut_a_bwd": lambda: lib.rcgan_shortcut_a_bwd(hd, n, h, w, c, L.F32, p(y), p(dx), 1),
    }
    out = {}
    for rep in range(REPS):
        for name, fn in forms.items():
            for _ in range(20):
                fn()
            ctx.event_record(2)
            for _ in range(iters):
                fn()
            ctx.event_record(3)
            ctx.sync()
            out.setdefault(name, []).append(1e3 * ctx.event_elapsed_ms(2, 3) / iters)
    return {k: dict(us_median=statistics.median(v), us_all=v) for k, v in out.items()}


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "classifier_step.json"))
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--precision", default="highest")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--add-stats", default=None)
    a = ap.parse_args()
    if a.add_stats is not None:
        rows = list(csv.DictReader(open(a.add_stats)))
        name_k = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
        dur_k = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
        tot = sum(float(r[dur_k]) for r in rows)
        gemm = sum(float(r[dur_k]) for r in rows if GEMM in r[name_k])
        top = sorted(rows, key=lambda r: -float(r[dur_k]))[:10]
        res = load(a.out)
        res["kernel_trace"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own (--trace): warm-up and timed steps alike",
                                   gather_gemm_share=gemm / tot, gather_gemm_launches=sum(int(r["Calls"]) for r in rows if GEMM in r[name_k]),
                                   total_gpu_ms=tot / 1e6, top10=[dict(kernel=r[name_k][:120], share=float(r[dur_k]) / tot) for r in top])
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
        print("gather GEMM share of the traced GPU time: %.3f" % (gemm / tot))
        return
    t = trainer(a.classes, a.precision)
    if a.trace:
        for _ in range(WARMUP + a.iters):
            t.step(0.1)
        t.ctx.sync()
        t.close()
        return
    from rcgan_amd import _lib as L
    ms = time_steps(t)
    res = load(a.out)
    res.update(what="LabelClassifierTrainer step (augment, forward, loss, backward, update), captured and replayed, fp32",
               batch=B, classes=a.classes, f32_matmul_precision=a.precision, warmup=WARMUP, steps=STEPS, repetitions=REPS,
               ms_per_step=statistics.median(ms), ms_per_step_all=ms, images_per_s=B / (statistics.median(ms) * 1e-3),
               source_hash=L.source_hash(),
               shortcut={"128x32x32x16": time_shortcut(t.ctx, B, 32, 32, 16), "128x16x16x32": time_shortcut(t.ctx, B, 16, 16, 32)})
    t.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("ms_per_step", "images_per_s", "ms_per_step_all")}))
    print(json.dumps(res["shortcut"]))


if __name__ == "__main__":
    main()
