#!/usr/bin/env python3
"""The CIFAR-10 (K = 10) and CIFAR-100 (K = 100) iterations of the engine in ONE process, alternating the two: B = 64, bf16, rcgan,
the bench.py iteration (G step + N_CRITIC critic steps), synthetic uniform batches.  K = 100 takes the kernels' wide routes
(per-class batch-norm reduction, unridden projection head).

usage: python scripts/bench_classes.py [--iters 20] [--repeats 5] [--out FILE]
"""
import argparse
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

B = 64


def build_pool(m, K, alpha=0.6):
    """bench.build_pool for K classes (uniform images: the step's cost does not depend on their content)."""
    from rcgan_amd import data as D
    from rcgan_amd.cifar import N_CRITIC
    P = bench.POOL
    rs = np.random.RandomState(1234)
    n = P * B
    clean = rs.randint(K, size=n)
    images = rs.randint(0, 256, size=(n, 3072))
    lab, rnd, bia, inv = D.corrupt_labels(clean, D.C_ALPHA(alpha, K), rs, n_classes=K)
    rs2 = np.random.RandomState(99)
    lg, bg = rs2.randint(K, size=(P, 2 * B)), rs2.randint(K, size=(P, 2 * B))
    fd, fg = [], []
    for k in range(P):
        s = slice(k * B, (k + 1) * B)
        fd.append(m.pack_feed("d", images=images[s], labels=lab[s], labels_random=rnd[s], labels_biased=bia[s], inv_weights=inv[s],
                              labels_all=np.concatenate([lab[s], bia[s]])))
        fg.append(m.pack_feed("g", labels_random_G=lg[k], labels_biased_G=bg[k]))
    dev = m.ctx.device
    lr = rnd[:n].reshape(P, B)
    pool = dict(feed_d=torch.from_numpy(np.stack(fd)).to(dev), feed_g=torch.from_numpy(np.stack(fg)).to(dev),
                feed_gf=torch.from_numpy(np.stack([m.pack_feed("gf", labels_random_all=np.concatenate([lr[(s0 + t) % P] for t in range(N_CRITIC)]))
                                                   for s0 in range(P)])).to(dev))
    torch.cuda.synchronize()
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rcgan_amd.cifar import CifarRCGAN
    runs = {}
    for K in (10, 100):
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=0, n_classes=K)
        runs[K] = dict(m=m, pool=build_pool(m, K), it=0, dc=[0], ms=[])

    def go(r, n):
        for _ in range(n):
            bench.iteration(r["m"], r["pool"], r["it"], r["dc"])
            r["it"] += 1
        torch.cuda.synchronize()
    for r in runs.values():
        go(r, 5)                     # warm-up: code objects, graph capture
    for _ in range(a.repeats):
        for r in runs.values():      # alternate the two models
            t0 = time.perf_counter()
            go(r, a.iters)
            r["ms"].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"batch": B, "dtype": "bf16", "algorithm": "rcgan", "iters_per_repeat": a.iters}
    for K, r in runs.items():
        out["K%d" % K] = dict(ms_per_iter_median=statistics.median(r["ms"]), min=min(r["ms"]), max=max(r["ms"]), all=r["ms"])
        r["m"].ctx.close()
    out["overhead_pct"] = 100.0 * (out["K100"]["ms_per_iter_median"] / out["K10"]["ms_per_iter_median"] - 1.0)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
