#!/usr/bin/env python3
"""The bench.py iteration (G step + N_CRITIC critic steps) with balanced consistency regularisation off and on (--bcr_real 10
--bcr_fake 10, translation), the engines alternating in ONE process: B = 64, bf16, rcgan, K = 10, synthetic uniform batches, the draws
on the device.  Same warm-up and repetition scheme as bench_lecam.py.

With the option on a critic step (a) runs the trunk on 4B rows instead of 2B and (b) leaves the fused head for the op-by-op route.  A
third engine, option off under RCGAN_FUSED_HEAD=0 (which takes the critic AND the generator step off the fused head), separates the
two: unfused - plain is the head route's share, bcr - unfused what the second half of the batch and the term itself add.

Beside the times: the calls of the C ABI that one iteration makes (counted on further engines that run the same bodies launch by
launch, use_graphs=False, because a replayed graph makes no calls).

usage: python scripts/bench_bcr.py [--iters 20] [--repeats 5] [--out FILE]      (default: profiles/bcr.json)
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

# name -> (constructor options, environment while the engine is constructed: RCGAN_FUSED_HEAD is read there)
ENGINES = {"plain": (dict(), {}),
           "unfused": (dict(), {"RCGAN_FUSED_HEAD": "0"}),
           "bcr": (dict(bcr_real=10.0, bcr_fake=10.0, bcr_policy="translation"), {})}


class _env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcr.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.cifar import CifarRCGAN
    counts, runs = {}, {}
    for name, (kw, env) in ENGINES.items():
        with _env(env):
            counts[name] = calls_per_iteration(kw)
            m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, **kw)
        assert m.fused_head == (name != "unfused") and m.bcr == (name == "bcr")
        runs[name] = dict(m=m, pool=build_pool(m, 10), it=0, dc=[0], ms=[])

    def go(r, n):
        for _ in range(n):
            bench.iteration(r["m"], r["pool"], r["it"], r["dc"])
            r["it"] += 1
        torch.cuda.synchronize()
    for r in runs.values():
        go(r, 5)                     # warm-up: code objects, graph capture
    for _ in range(a.repeats):
        for r in runs.values():      # alternate the engines
            t0 = time.perf_counter()
            go(r, a.iters)
            r["ms"].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"batch": B, "dtype": "bf16", "algorithm": "rcgan", "iters_per_repeat": a.iters, "kernel_source_hash": L.source_hash()}
    for name, r in runs.items():
        out[name] = dict(options=dict(ENGINES[name][0]), env=dict(ENGINES[name][1]), ms_per_iter_median=statistics.median(r["ms"]),
                         ms_per_iter_mean=statistics.mean(r["ms"]), min=min(r["ms"]), max=max(r["ms"]), all=r["ms"],
                         abi_calls_per_iteration=sum(counts[name].values()), bcr=r["m"].bcr_report(),
                         arena_bytes=r["m"].ctx.arena.cap, arena_peak_bytes=r["m"].ctx.arena.peak)
        r["m"].ctx.close()

    def added(x, y):
        diffs = [q - p for p, q in zip(out[x]["all"], out[y]["all"])]      # per repeat, the engines having run back to back
        delta = collections.Counter(counts[y])
        delta.subtract(counts[x])
        return dict(ms_per_iter=out[y]["ms_per_iter_mean"] - out[x]["ms_per_iter_mean"],
                    pct=100.0 * (out[y]["ms_per_iter_mean"] - out[x]["ms_per_iter_mean"]) / out[x]["ms_per_iter_mean"],
                    by_repeat=dict(median=statistics.median(diffs), min=min(diffs), max=max(diffs), all=diffs),
                    abi_calls_per_iteration=out[y]["abi_calls_per_iteration"] - out[x]["abi_calls_per_iteration"],
                    abi_call_difference={k: v for k, v in sorted(delta.items()) if v})
    out["added_by_the_option"] = added("plain", "bcr")
    out["added_by_the_unfused_head"] = added("plain", "unfused")
    out["added_over_the_unfused_head"] = added("unfused", "bcr")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
