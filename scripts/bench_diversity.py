#!/usr/bin/env python3
"""The bench.py iteration (G step + N_CRITIC critic steps) with the diversity-sensitive generator term off and on (--diversity 1
--diversity_tau 0.8), the two engines alternating in ONE process: B = 64, bf16, rcgan, K = 10, synthetic uniform batches, the draws
on the device.  Same warm-up and repetition scheme as bench_lecam.py.  Both engines are fed generator labels paired as
train_cifar.py pairs them (rows B..2B of labels_random_G repeat rows 0..B): with unpaired labels nine pairs in ten would be masked
and write no gradient, which is not the cost of a run that uses the option.

Beside the times: the calls of the C ABI that one iteration makes in both states (counted launch by launch, use_graphs=False), and
-- with --parent-root DIR, a built checkout of the parent commit -- bench.py of this tree (the option off) against bench.py of the
parent, alternating as child processes.

usage: python scripts/bench_diversity.py [--iters 20] [--repeats 5] [--parent-root DIR] [--out FILE]   (default: profiles/diversity.json)
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
from bench_ada import CountingLib  # noqa: E402
from bench_classes import B, build_pool  # noqa: E402
from bench_frechet import bench_ms  # noqa: E402

ENGINES = {"plain": dict(), "diversity": dict(diversity=1.0, diversity_tau=0.8)}


def paired_pool(m):
    """build_pool with every generator batch's labels_random_G paired: the packed "g" feed is [labels_random_G (2B) ; labels_biased_G
    (2B)] int32 words, and words B..2B take words 0..B (cifar.pair_generator_labels on the device copy)."""
    assert [f[0] for f in m.feed_layout["g"]] == ["labels_random_G", "labels_biased_G"]
    pool = build_pool(m, 10)
    pool["feed_g"][:, B:2 * B] = pool["feed_g"][:, :B]
    torch.cuda.synchronize()
    return pool


def calls_per_iteration(kw):
    """-> {entry point: calls} of one steady-state iteration, launch by launch."""
    from rcgan_amd.cifar import CifarRCGAN
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, use_graphs=False, **kw)
    try:
        pool, dc = paired_pool(m), [0]
        for it in range(2):
            bench.iteration(m, pool, it, dc)
        torch.cuda.synchronize()
        lib = m.ctx.lib
        m.ctx.lib = CountingLib(lib)
        try:
            bench.iteration(m, pool, 2, dc)
            calls = dict(m.ctx.lib.calls)
        finally:
            m.ctx.lib = lib
        torch.cuda.synchronize()
        return calls
    finally:
        m.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversity.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.cifar import CifarRCGAN
    counts = {name: calls_per_iteration(kw) for name, kw in ENGINES.items()}
    runs = {}
    for name, kw in ENGINES.items():
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, **kw)
        runs[name] = dict(m=m, pool=paired_pool(m), it=0, dc=[0], ms=[])

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
                         diversity=r["m"].diversity_report())
        r["m"].ctx.close()
    a_, b_ = out["plain"], out["diversity"]
    out["added_ms_per_iter"] = b_["ms_per_iter_mean"] - a_["ms_per_iter_mean"]
    # the spread of the difference: per repeat, the engines having run back to back
    diffs = [y - x for x, y in zip(a_["all"], b_["all"])]
    out["added_ms_per_iter_by_repeat"] = dict(median=statistics.median(diffs), min=min(diffs), max=max(diffs), all=diffs)
    out["overhead_pct"] = 100.0 * out["added_ms_per_iter"] / a_["ms_per_iter_mean"]
    out["added_abi_calls_per_iteration"] = b_["abi_calls_per_iteration"] - a_["abi_calls_per_iteration"]
    delta = collections.Counter(counts["diversity"])
    delta.subtract(counts["plain"])
    out["abi_call_difference"] = {k: v for k, v in sorted(delta.items()) if v}
    # the option off against the parent commit: bench.py of both trees, alternating
    roots = {"this_tree": ROOT}
    if a.parent_root:
        roots["parent_commit"] = os.path.abspath(a.parent_root)
    ms = {name: [] for name in roots}
    for _ in range(a.bench_repeats):
        for name, root in roots.items():
            ms[name].append(bench_ms(root, a.bench_steps, 10))
    out["training_iteration_option_off"] = {name: dict(ms_per_iter_median=statistics.median(v), all=v) for name, v in ms.items()}
    if not a.parent_root:
        out["training_iteration_option_off"]["parent_commit"] = "not measured (no --parent-root)"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
