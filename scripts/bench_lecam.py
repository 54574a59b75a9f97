#!/usr/bin/env python3
"""The bench.py iteration (G step + N_CRITIC critic steps) with the LeCam regulariser off and on (--lecam 0.3 --lecam_decay 0.99), the
two engines alternating in ONE process: B = 64, bf16, rcgan, K = 10, synthetic uniform batches, the draws on the device.  Same warm-up
and repetition scheme as bench_ada.py.

Beside the times: the calls of the C ABI that one iteration makes (every entry point that enqueues work is one call per op; counted
on a third and fourth engine that run the same bodies launch by launch, use_graphs=False, because a replayed graph makes no calls).

usage: python scripts/bench_lecam.py [--iters 20] [--repeats 5] [--out FILE]      (default: profiles/lecam.json)
"""
import argparse
import collections
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
from bench_ada import calls_per_iteration  # noqa: E402
from bench_classes import B, build_pool  # noqa: E402

ENGINES = {"plain": dict(), "lecam": dict(lecam=0.3, lecam_decay=0.99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lecam.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.cifar import CifarRCGAN
    counts = {name: calls_per_iteration(kw) for name, kw in ENGINES.items()}
    runs = {}
    for name, kw in ENGINES.items():
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, **kw)
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
        out[name] = dict(options=dict(ENGINES[name]), ms_per_iter_median=statistics.median(r["ms"]), ms_per_iter_mean=statistics.mean(r["ms"]),
                         min=min(r["ms"]), max=max(r["ms"]), all=r["ms"], abi_calls_per_iteration=sum(counts[name].values()),
                         lecam=r["m"].lecam_report())
        r["m"].ctx.close()
    a_, b_ = out["plain"], out["lecam"]
    out["added_ms_per_iter"] = b_["ms_per_iter_mean"] - a_["ms_per_iter_mean"]
    # the spread of the difference: per repeat, the engines having run back to back
    diffs = [y - x for x, y in zip(a_["all"], b_["all"])]
    out["added_ms_per_iter_by_repeat"] = dict(median=statistics.median(diffs), min=min(diffs), max=max(diffs), all=diffs)
    out["overhead_pct"] = 100.0 * out["added_ms_per_iter"] / a_["ms_per_iter_mean"]
    out["added_abi_calls_per_iteration"] = b_["abi_calls_per_iteration"] - a_["abi_calls_per_iteration"]
    delta = collections.Counter(counts["lecam"])
    delta.subtract(counts["plain"])
    out["abi_call_difference"] = {k: v for k, v in sorted(delta.items()) if v}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
