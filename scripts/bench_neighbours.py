#!/usr/bin/env python3
"""Cost of the nearest-training-image metrics (--neighbours_freq of train_cifar.py) and what they separate, one MI355X:

  * rcgan_nn_u8 per call (HIP events around a train of calls, after a warm-up) on random uint8 rows at 10 000 x 50 000 x 3072 pooled
    and in 10 equal segments, 50 000 x 50 000 x 3072 of one set against itself with exclusion, and 10 000 x 60 000 x 784; for each
    the achieved int8 rate (2 nq nr d operations over the pairs that meet) beside the dense int8 matrix peak (twice the bf16 one);
  * wall time of ONE NeighbourEvaluator.evaluate of 10 000 generated images against 50 000 training and 10 000 held-out template
    images, and the same evaluation again with every part followed by a synchronisation: host (layout, sorting, statistics), upload,
    kernel, download;
  * what the numbers separate (the sets of tests/test_gpu_neighbours.py: 3000 training images, 600 per set);
  * the training iteration with the flag off: bench.py of this tree, and of a built checkout of the parent commit when
    --parent-root DIR names one, the two alternating as child processes.

usage: python scripts/bench_neighbours.py [--samples 10000] [--train 50000] [--repeats 3] [--parent-root DIR] [--out FILE]
(default: profiles/neighbours.json)
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
I8_PEAK_TOPS = 5000.0        # dense int8 matrix peak: twice the ~2.5 PF bf16 one (the same cycles per instruction at twice the K)


def kernel(ctx, nq, nr, d, n_seg, same=False):
    import torch
    from rcgan_amd import neighbours as NB
    g = torch.Generator(device=ctx.device)
    g.manual_seed(1)
    r = torch.randint(0, 256, (nr, d), dtype=torch.uint8, device=ctx.device, generator=g)
    q = r if same else torch.randint(0, 256, (nq, d), dtype=torch.uint8, device=ctx.device, generator=g)
    off = lambda n: torch.from_numpy(np.round(np.linspace(0, n, n_seg + 1)).astype(np.int32)).to(ctx.device)
    q_off, r_off = off(nq), off(nr)
    torch.cuda.synchronize()
    t = timed_calls(ctx, lambda: NB.nn_u8(ctx, q, q_off, r, r_off, same))
    qo, ro = q_off.cpu().numpy().astype(np.int64), r_off.cpu().numpy().astype(np.int64)
    ops = 2.0 * d * float(((qo[1:] - qo[:-1]) * (ro[1:] - ro[:-1])).sum())
    tops = ops / (t["ms_per_call_median"] * 1e-3) / 1e12
    t.update(nq=nq, nr=nr, d=d, segments=n_seg, exclude_same_row=bool(same), int8_tera_ops=ops / 1e12, achieved_int8_tops=tops,
             int8_matrix_peak_tops=I8_PEAK_TOPS, share_of_peak=tops / I8_PEAK_TOPS)
    return t


def evaluation(train, samples, repeats):
    from rcgan_amd import data as D
    from rcgan_amd import neighbours as NB
    tx, ty = D.synthetic_cifar(train, 1234, "templates")
    hx, hy = D.synthetic_cifar(samples, 1235, "templates")
    gx, gy = D.synthetic_cifar(samples, 1236, "templates")
    ev = NB.NeighbourEvaluator(K)
    t0 = time.perf_counter()
    ev.prepare_real(tx, ty, hx, hy)
    real_s = time.perf_counter() - t0
    plain = []
    for rep in range(repeats + 1):                 # the first one warms up (code object, allocator) and is dropped
        ev.ctx.sync()
        t0 = time.perf_counter()
        r = ev.evaluate(gx, gy)
        if rep:
            plain.append(time.perf_counter() - t0)
    # the same evaluation with a synchronisation behind every part
    spent = dict(host_layout_s=0.0, upload_s=0.0, kernel_s=0.0, download_s=0.0)
    saved = NB.as_rows, NB.ImageSet.__init__, NB.nn_u8, NB.download

    def timed(key, fn, inner=None):
        def go(*a, **kw):
            ev.ctx.sync()
            t = time.perf_counter()
            before = spent[inner] if inner else 0.0
            out = fn(*a, **kw)
            ev.ctx.sync()
            spent[key] += time.perf_counter() - t - ((spent[inner] - before) if inner else 0.0)
            return out
        return go
    NB.as_rows = timed("host_layout_s", saved[0])
    NB.ImageSet.__init__ = timed("upload_s", saved[1], inner="host_layout_s")
    NB.nn_u8 = timed("kernel_s", saved[2])
    NB.download = timed("download_s", saved[3])
    try:
        ev.ctx.sync()
        t0 = time.perf_counter()
        ev.evaluate(gx, gy)
        split_s = time.perf_counter() - t0
    finally:
        NB.as_rows, NB.ImageSet.__init__, NB.nn_u8, NB.download = saved
    spent["host_statistics_s"] = split_s - sum(spent.values())
    res = dict(evaluate_s=statistics.median(plain), all=plain, evaluate_with_a_synchronisation_per_part_s=split_s, parts=spent,
               training_images=len(tx), heldout_images=len(hx), samples=len(gx), prepare_real_s=real_s,
               result={k: r[k] for k in NB.SCALARS + ("classes_above_heldout", "classes_compared", "classes_used", "loo_rows")})
    ev.close()
    return res


def separation():
    from rcgan_amd import data as D
    from rcgan_amd import neighbours as NB
    noisy = lambda rs, x: np.clip(np.rint(x.astype(np.float64) + 2.0 * rs.randn(*x.shape)), 0, 255).astype(np.uint8)
    T, lt = D.synthetic_cifar(3000, 1234, "templates")
    H, lh = D.synthetic_cifar(600, 1235, "templates")
    F, lf = D.synthetic_cifar(600, 1236, "templates")
    rs = np.random.RandomState(7)
    pick = np.sort(rs.permutation(len(T))[:600])
    C, lc = noisy(rs, T[pick]), lt[pick]
    one = D.template_images(np.random.RandomState(33), np.arange(K)).astype(np.uint8)
    lab = np.arange(600) % K
    sets = dict(fresh_draw=(F, lf), noisy_copies=(C, lc), half_fresh_half_copies=(np.concatenate([F[:300], C[:300]]), np.concatenate([lf[:300], lc[:300]])),
                collapsed=(noisy(rs, one[lab]), lab))
    ev = NB.NeighbourEvaluator(K)
    ev.prepare_real(T, lt, H, lh)
    out = dict(training_images=len(T), heldout_images=len(H), images_per_set=600)
    for name, (x, labels) in sets.items():
        r = ev.evaluate(x, labels)
        out[name] = {k: r[k] for k in NB.SCALARS + ("classes_above_heldout", "classes_compared", "classes_used")}
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--train", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash()}
    ctx = Context(0, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
    out["kernel_pooled_3072"] = kernel(ctx, a.samples, a.train, 3072, 1)
    out["kernel_10_classes_3072"] = kernel(ctx, a.samples, a.train, 3072, 10)
    out["kernel_train_against_itself_3072"] = kernel(ctx, a.train, a.train, 3072, 1, same=True)
    out["kernel_pooled_784"] = kernel(ctx, a.samples, 60000, 784, 1)
    ctx.close()
    print("kernel timed", file=sys.stderr, flush=True)
    out["evaluation"] = evaluation(a.train, a.samples, a.repeats)
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
