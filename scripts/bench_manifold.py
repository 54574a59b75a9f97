#!/usr/bin/env python3
"""Cost of the k-NN precision / recall / density / coverage metric (--prdc_freq of train_cifar.py), one MI355X:

  * rcgan_knn_radius and rcgan_ball_query per call, d = 64, k = 5 (HIP events around a train of calls, after a warm-up), at
    10 000 x 10 000 rows pooled, the same rows as 10 and as 100 equal classes, and 50 000 rows against themselves;
  * wall time of ONE ManifoldEvaluator.evaluate of 10 000 generated images against 10 000 real ones (frozen features, upload, the six
    launches of both layouts, one download, the host arithmetic), and of the classifier's feature pass over the same images alone:
    the two kernels of one evaluation should cost less than that pass, or the metric and not the network prices an evaluation;
  * tests/manifold_ref.py's float64 host computation of the same four numbers at 10 000 x 10 000 (its thread pool: 16 cores at most);
  * the training iteration with the flag off: bench.py of this tree, and of a checkout of the parent commit when --parent-root DIR
    names one (built), the two alternating as child processes.

usage: python scripts/bench_manifold.py [--samples 10000] [--repeats 3] [--parent-root DIR] [--out FILE]   (default: profiles/manifold.json)
"""
import argparse
import ctypes as C
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

D, KNN = 64, 5


def timed_calls(ctx, go, window_ms=300.0):
    """Median, min and max over 5 trains of launches, milliseconds per call (HIP events on the context's stream).  A warm-up first;
    a train is as many calls as fill about ``window_ms`` (sized from a first short train, at least 3)."""
    for _ in range(3):
        go()
    ctx.sync()
    ctx.event_record(0)
    for _ in range(3):
        go()
    ctx.event_record(1)
    ctx.sync()
    calls = int(max(3, min(5000, window_ms / max(ctx.event_elapsed_ms(0, 1) / 3, 1e-3))))
    ms = []
    for _ in range(5):
        ctx.event_record(0)
        for _ in range(calls):
            go()
        ctx.event_record(1)
        ctx.sync()
        ms.append(ctx.event_elapsed_ms(0, 1) / calls)
    return dict(ms_per_call_median=statistics.median(ms), min=min(ms), max=max(ms), calls_per_train=calls)


def kernels(ctx, nq, nr, n_seg, same_set=False):
    """Both entries at [nq] queries x [nr] references in n_seg equal segments; same_set: the radius search of a set against itself only."""
    from rcgan_amd import manifold as MF
    rs = np.random.RandomState(1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    off = lambda n: up(np.round(np.linspace(0, n, n_seg + 1)).astype(np.int32))
    r, r_off = up(rs.randn(nr, D).astype(np.float32)), off(nr)
    torch.cuda.synchronize()
    rad = MF.knn_radius(ctx, r, r_off, KNN)
    out = dict(nq=nq, nr=nr, d=D, k=KNN, segments=n_seg)
    p = lambda t: C.c_void_p(t.data_ptr())
    out["knn_radius"] = timed_calls(ctx, lambda: ctx.check(ctx.lib.rcgan_knn_radius(ctx.h, nr, D, KNN, n_seg, p(r), p(r_off), p(rad))))
    out["knn_radius"]["pair_distances_per_s"] = float(nr) * nr / n_seg / (out["knn_radius"]["ms_per_call_median"] * 1e-3)
    if not same_set:
        q, q_off = up((1.1 * rs.randn(nq, D) + 0.2).astype(np.float32)), off(nq)
        cnt = torch.empty(nq, dtype=torch.int32, device=ctx.device)
        near = torch.empty(nq, dtype=torch.float32, device=ctx.device)
        torch.cuda.synchronize()
        go = lambda: ctx.check(ctx.lib.rcgan_ball_query(ctx.h, nq, nr, D, n_seg, p(q), p(q_off), p(r), p(r_off), p(rad), p(cnt), p(near)))
        out["ball_query"] = timed_calls(ctx, go)
        out["ball_query"]["pair_distances_per_s"] = float(nq) * nr / n_seg / (out["ball_query"]["ms_per_call_median"] * 1e-3)
    return out


def evaluation(samples, repeats, K=10):
    """One evaluate() of ``samples`` generated images against as many real (template) images; the feature pass over the same images."""
    from rcgan_amd import data as DT
    from rcgan_amd import manifold as MF
    from rcgan_amd.cifar import Z_DIM, CifarRCGAN
    from rcgan_amd.train_cifar import gen_acc_label_lists
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=64, dtype="bf16", seed=0, n_classes=K)
    rs = np.random.RandomState(0)
    balanced = gen_acc_label_lists(K, balanced=True)
    calls = [balanced[j % len(balanced)] for j in range(samples // 100)]
    x = [m.sample(labels, rs.normal(size=(100, Z_DIM)).astype('float32')) for labels in calls]
    x = ((np.concatenate(x, axis=0) + 1.) * (255.99 / 2)).astype('int32').reshape((-1, 32, 32, 3))
    labels = np.concatenate(calls, axis=0)
    m.ctx.close()
    ev = MF.ManifoldEvaluator(K, k=KNN)
    rx, ry = DT.synthetic_cifar(samples, 1234, "templates", K)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    real_s = time.perf_counter() - t0
    rows = []
    for rep in range(repeats + 1):                 # the first one warms up (code objects, allocator) and is dropped
        t0 = time.perf_counter()
        r = ev.evaluate(x, labels)
        t1 = time.perf_counter()
        feat = ev.clf.features(x, chunk=ev.chunk)  # (ends in a download: synchronised)
        t2 = time.perf_counter()
        if rep:
            rows.append(dict(evaluate_s=t1 - t0, feature_pass_s=t2 - t1))
    out = {k: statistics.median(r_[k] for r_ in rows) for k in rows[0]}
    out.update(samples=len(x), real_images=len(rx), prepare_real_s=real_s, classes_used=r["classes_used"],
               all_evaluate_s=[r_["evaluate_s"] for r_ in rows], all_feature_pass_s=[r_["feature_pass_s"] for r_ in rows],
               pooled={k: r[k] for k in MF.METRICS})
    real_feat = ev.real.pooled.cpu().numpy()
    ev.close()
    return out, real_feat, feat


def host_reference(real_feat, gen_feat):
    from tests import manifold_ref as MR
    t0 = time.perf_counter()
    r = MR.metrics_of(real_feat, gen_feat, KNN)
    return dict(rows=[len(real_feat), len(gen_feat)], d=int(real_feat.shape[1]), seconds=time.perf_counter() - t0, threads=MR.THREADS, pooled=r)


def bench_ms(root, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--no-cpu-baseline"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, check=True)
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--no-host-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifold.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash(), "generator_dtype": "bf16", "classifier_dtype": "f32", "d": D, "k": KNN}
    n = a.samples
    ctx = Context(0, "f32", arena_bytes=1 << 26, ws_bytes=1 << 20)
    out["kernels_pooled"] = kernels(ctx, n, n, 1)
    out["kernels_10_classes"] = kernels(ctx, n, n, 10)
    out["kernels_100_classes"] = kernels(ctx, n, n, 100)
    out["kernels_real_set_self_search"] = kernels(ctx, 5 * n, 5 * n, 1, same_set=True)
    ctx.close()
    out["evaluation"], real_feat, gen_feat = evaluation(n, a.repeats)
    # one evaluation launches, per layout, one radius search of the generated set and two ball queries
    per = lambda key: out[key]["knn_radius"]["ms_per_call_median"] + 2 * out[key]["ball_query"]["ms_per_call_median"]
    kernels_ms = per("kernels_pooled") + per("kernels_10_classes")
    feature_ms = out["evaluation"]["feature_pass_s"] * 1e3
    out["kernels_against_the_feature_pass"] = dict(
        kernels_of_one_evaluation_ms=kernels_ms, feature_pass_ms=feature_ms, kernels_cost_less=bool(kernels_ms < feature_ms),
        note="the six launches of one evaluation (pooled + 10 classes, from the per-call medians above) against the frozen feature pass over "
             "the same %d images" % n)
    out["host_float64_reference"] = "not measured (--no-host-reference)" if a.no_host_reference else host_reference(real_feat, gen_feat)
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
