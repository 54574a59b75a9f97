#!/usr/bin/env python3
"""The bench.py iteration (G step + N_CRITIC critic steps) with DiffAugment off and with color,translation,cutout, the two engines
alternating in ONE process: B = 64, bf16, rcgan, K = 10, synthetic uniform batches, the draws on the device.

usage: python scripts/bench_diffaugment.py [--iters 20] [--repeats 5] [--out FILE]      (default: profiles/diffaugment.json)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench  # noqa: E402
import rcgan_amd  # noqa: E402,F401
from bench_classes import B, build_pool  # noqa: E402

POLICIES = {"off": "", "color_translation_cutout": "color,translation,cutout"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffaugment.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.cifar import CifarRCGAN
    runs = {}
    for name, policy in POLICIES.items():
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, diffaugment=policy)
        runs[name] = dict(m=m, pool=build_pool(m, 10), it=0, dc=[0], ms=[])

    def go(r, n):
        for _ in range(n):
            bench.iteration(r["m"], r["pool"], r["it"], r["dc"])
            r["it"] += 1
        torch.cuda.synchronize()
    for r in runs.values():
        go(r, 5)                     # warm-up: code objects, graph capture
    for _ in range(a.repeats):
        for r in runs.values():      # alternate the two engines
            t0 = time.perf_counter()
            go(r, a.iters)
            r["ms"].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"batch": B, "dtype": "bf16", "algorithm": "rcgan", "iters_per_repeat": a.iters, "kernel_source_hash": L.source_hash()}
    for name, r in runs.items():
        out[name] = dict(policy=POLICIES[name], ms_per_iter_median=statistics.median(r["ms"]), min=min(r["ms"]), max=max(r["ms"]), all=r["ms"])
        r["m"].ctx.close()
    out["added_ms_per_iter"] = out["color_translation_cutout"]["ms_per_iter_median"] - out["off"]["ms_per_iter_median"]
    out["overhead_pct"] = 100.0 * out["added_ms_per_iter"] / out["off"]["ms_per_iter_median"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
