#!/usr/bin/env python3
"""Cost of the kernel distance (--kid_freq of train_cifar.py) and what it separates, one MI355X:

  * rcgan_poly3_rowsum per call, d = 64 (HIP events around a train of calls, after a warm-up), at 10 000 x 10 000 rows pooled, the
    same rows as 10 and as 100 equal classes, and 50 000 rows against themselves without the diagonal; in the same process,
    alternating with it, rcgan_ball_query -- the project's vector-unit kernel for the same pair count -- at the same shapes;
  * wall time of ONE KernelDistanceEvaluator.evaluate of 10 000 generated images against 10 000 real ones, split into the feature
    pass (frozen features, upload) and the metric (six launches, one download, the host arithmetic);
  * what the numbers separate, in the setting of the Frechet subsection of DESIGN.md (512 calibration images, 2048 template images
    per set): two independent draws, a set of classes 0-4 only, uniform noise, and the second draw with its labels shifted by one;
  * the training iteration with the flag off: bench.py of this tree, and of a checkout of the parent commit when --parent-root DIR
    names one (built), the two alternating as child processes.

usage: python scripts/bench_kid.py [--samples 10000] [--repeats 3] [--parent-root DIR] [--out FILE]   (default: profiles/kid.json)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rcgan_amd  # noqa: E402,F401
from bench_manifold import bench_ms, timed_calls  # noqa: E402

D = 64


def kernels(ctx, nq, nr, n_seg, same_set=False, rounds=3):
    """rcgan_poly3_rowsum and rcgan_ball_query at [nq] queries x [nr] references in n_seg equal segments, ``rounds`` times alternating;
    same_set: the rows against themselves, the diagonal left out of the kernel sum."""
    from rcgan_amd import kid as KD
    from rcgan_amd import manifold as MF
    rs = np.random.RandomState(1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    off = lambda n: up(np.round(np.linspace(0, n, n_seg + 1)).astype(np.int32))
    r, r_off = up(np.abs(rs.randn(nr, D)).astype(np.float32)), off(nr)
    q, q_off = (r, r_off) if same_set else (up((1.1 * np.abs(rs.randn(nq, D)) + 0.2).astype(np.float32)), off(nq))
    torch.cuda.synchronize()
    rad = MF.knn_radius(ctx, r, r_off, 5)
    rowsum = torch.empty(nq, dtype=torch.float64, device=ctx.device)
    cnt = torch.empty(nq, dtype=torch.int32, device=ctx.device)
    near = torch.empty(nq, dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    go_poly = lambda: ctx.check(ctx.lib.rcgan_poly3_rowsum(ctx.h, nq, nr, D, n_seg, p(q), p(q_off), p(r), p(r_off), KD.gamma_of(D), KD.COEF0,
                                                           1 if same_set else 0, p(rowsum)))
    go_ball = lambda: ctx.check(ctx.lib.rcgan_ball_query(ctx.h, nq, nr, D, n_seg, p(q), p(q_off), p(r), p(r_off), p(rad), p(cnt), p(near)))
    poly, ball = [], []
    for _ in range(rounds):
        poly.append(timed_calls(ctx, go_poly))
        ball.append(timed_calls(ctx, go_ball))
    pairs = float(nq) * nr / n_seg

    def fold(rows):
        med = statistics.median(x["ms_per_call_median"] for x in rows)
        return dict(ms_per_call_median=med, min=min(x["min"] for x in rows), max=max(x["max"] for x in rows),
                    medians_of_the_rounds=[x["ms_per_call_median"] for x in rows], pairs_per_s=pairs / (med * 1e-3),
                    inner_product_tflops=2.0 * D * pairs / (med * 1e-3) / 1e12)
    out = dict(nq=nq, nr=nr, d=D, segments=n_seg, poly3_rowsum=fold(poly), ball_query=fold(ball))
    out["poly3_over_ball_query"] = out["poly3_rowsum"]["ms_per_call_median"] / out["ball_query"]["ms_per_call_median"]
    return out


def evaluation(samples, repeats, K=10):
    """One evaluate() of ``samples`` generated images against as many real (template) images: the feature pass and the metric apart."""
    from rcgan_amd import data as DT
    from rcgan_amd import kid as KD
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
    ev = KD.KernelDistanceEvaluator(K)
    rx, ry = DT.synthetic_cifar(samples, 1234, "templates", K)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    real_s = time.perf_counter() - t0
    rows = []
    for rep in range(repeats + 1):                 # the first one warms up (code objects, allocator) and is dropped
        t0 = time.perf_counter()
        r = ev.evaluate(x, labels)
        t1 = time.perf_counter()
        fs = ev.feature_set(x, labels)
        ev.clf.ctx.sync()
        t2 = time.perf_counter()
        KD.compare(ev.real, ev.real_sums, fs, ev.subset_size)          # (ends in a download: synchronised)
        t3 = time.perf_counter()
        if rep:
            rows.append(dict(evaluate_s=t1 - t0, feature_pass_s=t2 - t1, metric_s=t3 - t2))
    out = {k: statistics.median(r_[k] for r_ in rows) for k in rows[0]}
    out.update(samples=len(x), real_images=len(rx), prepare_real_s=real_s, all=rows,
               result={k: r[k] for k in ("kernel_distance", "intra_class_kernel_distance", "intra_class_kernel_distance_se", "subset_mean",
                                         "subset_std", "subsets", "classes_used")})
    ev.close()
    return out


def separation(n=2048, n_calibration=512, K=10):
    """Template images, the Frechet subsection's setting: what each number says about four generated sets against one real set."""
    from rcgan_amd import data as DT
    from rcgan_amd import kid as KD
    from rcgan_amd.eval_cifar import LabelClassifier

    def templates(seed, count, classes=K):
        rs = np.random.RandomState(seed)
        labels = rs.randint(classes, size=count)
        x = DT.template_images(rs, labels).reshape(count, 3, 32, 32).transpose(0, 2, 3, 1)
        return np.ascontiguousarray(x), labels
    clf = LabelClassifier(0, arena_bytes=2 << 30)
    clf.calibrate(templates(21, n_calibration)[0])
    ev = KD.KernelDistanceEvaluator(K, subset_size=256, chunk=256, clf=clf)
    ev.prepare_real(*templates(22, n))
    xb, lb = templates(23, n)
    rs = np.random.RandomState(25)
    sets = dict(independent_draw=(xb, lb), classes_0_to_4_only=templates(24, n, 5),
                uniform_noise=(rs.randint(0, 256, size=(n, 32, 32, 3)), rs.randint(K, size=n)), labels_shifted_by_one=(xb, (lb + 1) % K))
    keys = ("kernel_distance", "intra_class_kernel_distance", "intra_class_kernel_distance_se", "subset_mean", "subset_std", "subsets",
            "classes_used")
    out = dict(images_per_set=n, calibration_images=n_calibration, subset_size=256)
    for name, (x, labels) in sets.items():
        r = ev.evaluate(x, labels)
        out[name] = {k: r[k] for k in keys}
    ev.close()
    clf.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kid.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash(), "generator_dtype": "bf16", "classifier_dtype": "f32", "d": D}
    n = a.samples
    ctx = Context(0, "f32", arena_bytes=1 << 26, ws_bytes=1 << 20)
    out["kernels_pooled"] = kernels(ctx, n, n, 1)
    out["kernels_10_classes"] = kernels(ctx, n, n, 10)
    out["kernels_100_classes"] = kernels(ctx, n, n, 100)
    out["kernels_real_set_against_itself"] = kernels(ctx, 5 * n, 5 * n, 1, same_set=True)
    ctx.close()
    print("kernels timed", file=sys.stderr, flush=True)
    out["evaluation"] = evaluation(n, a.repeats)
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
