#!/usr/bin/env python3
"""Cost of the sliced Wasserstein distance (--swd_freq of train_cifar.py) and what it separates, one MI355X:

  * each of the four calls of csrc/swd.hip (HIP events around a train of calls, after a warm-up) at the default size -- 10 000
    images of 32x32x3 as one pooled segment, pyramid level 0 (49 descriptors per image, rows of 2^19 floats), as many directions
    as fit a 64 MiB projection buffer -- and the same calls in the per-class layout (10 segments);
  * wall time of ONE SwdEvaluator.evaluate at that size (10 000 generated against 20 000 real images, 128 directions), the first
    one (which also takes the floor) and the later ones;
  * the float64 restatement (tests/swd_ref.py) on the host for ``--ref-images`` images a side, pooled, and that time scaled to the
    evaluation's four comparisons (linear in the image count: its sort's logarithm is ignored);
  * what the number separates on template images (4 classes, 100 images per class, 128 directions): a second draw of the real
    distribution, the draw under shuffled labels, a collapsed set and a blurred set, per class and per level, with the floor;
  * the training iteration with the flag off: bench.py of this tree, and of a built checkout of the parent commit when
    --parent-root DIR names one, the two alternating as child processes.

usage: python scripts/bench_swd.py [--samples 10000] [--repeats 3] [--ref-images 500] [--parent-root DIR] [--out FILE]
(default: profiles/swd.json)
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


def templates(seed, labels):
    from rcgan_amd import data as DT
    rows = np.concatenate([DT.template_images(np.random.RandomState(seed + i), labels[i:i + 5000]) for i in range(0, len(labels), 5000)])
    return rows.astype(np.uint8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)


def calls(ctx, x, counts, level=0):
    """The four calls on images x (device-ready uint8 NHWC, sorted by segment) in segments of ``counts`` images."""
    import torch
    from rcgan_amd import swd as SW
    n, h, w, c = x.shape
    n_seg, n_pos = len(counts), SW.positions(h, w, level)
    width = SW.pow2_at_least(max(counts) * n_pos)
    nd = int(max(1, min(128, SW.BUFFER_BYTES // (n_seg * width * 4))))
    with torch.cuda.stream(ctx.stream):
        dx = torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(ctx.device)
        have = torch.from_numpy((np.asarray(counts) * n_pos).astype(np.int32)).to(ctx.device)
        dirs = torch.from_numpy(SW.directions(nd, c)[level]).to(ctx.device)
        pa = torch.empty((nd, n_seg, width), dtype=torch.float32, device=ctx.device)
        pb = torch.empty_like(pa)
        keep = torch.empty_like(pa)
        sums = torch.empty((nd, n_seg), dtype=torch.float64, device=ctx.device)
        other = dx.roll(1, 0).contiguous()         # (a second set for the other side of the row sums)
    mom = SW.swd_moments(ctx, dx, off, level)
    SW.swd_project(ctx, dx, off, mom, dirs, level, width, out=keep)
    SW.swd_project(ctx, other, off, mom, dirs, level, width, out=pb)
    out = dict(images=n, segments=n_seg, level=level, descriptors_per_image=n_pos, row_width=width, directions_per_chunk=nd,
               projection_buffer_mib=nd * n_seg * width * 4 / 2.0 ** 20)
    out["moments"] = timed_calls(ctx, lambda: SW.swd_moments(ctx, dx, off, level))
    out["project"] = timed_calls(ctx, lambda: SW.swd_project(ctx, dx, off, mom, dirs, level, width, out=pa))

    def sort():                                   # (a sort of sorted rows would be a different workload: restore the projections first)
        pa.copy_(keep)
        SW.sort_rows(ctx, pa, nd * n_seg, width)
    with torch.cuda.stream(ctx.stream):
        both = timed_calls(ctx, sort)
        copy = timed_calls(ctx, lambda: pa.copy_(keep))
    out["sort_rows"] = dict(ms_per_call_median=both["ms_per_call_median"] - copy["ms_per_call_median"], with_restoring_copy=both, restoring_copy=copy)
    SW.sort_rows(ctx, pb, nd * n_seg, width)
    out["absdiff_rowsum"] = timed_calls(ctx, lambda: SW.absdiff_rowsum(ctx, pa, pb, have, nd * n_seg, width, sums))
    return out


def evaluation(samples, repeats, ref_images):
    from rcgan_amd import swd as SW
    from tests import swd_ref as SR
    ry, gy = np.arange(2 * samples) % K, np.arange(samples) % K
    rx, gx = templates(1234, ry), templates(4321, gy)
    ev = SW.SwdEvaluator(K)
    t0 = time.perf_counter()
    ev.prepare_real(rx, ry)
    ev.ctx.sync()
    real_s = time.perf_counter() - t0
    times = []
    for rep in range(repeats + 1):                 # the first one also takes the floor (and warms up code objects and the allocator)
        ev.ctx.sync()
        t0 = time.perf_counter()
        r = ev.evaluate(gx, gy)
        times.append(time.perf_counter() - t0)
    res = dict(samples=samples, real_images=len(rx), directions=ev.directions, prepare_real_s=real_s, first_evaluate_with_floor_s=times[0],
               evaluate_s=statistics.median(times[1:]), all=times, result=SW.json_ready(r))
    dirs = ev.host_dirs
    ev.close()
    m = ref_images
    t0 = time.perf_counter()
    want = SR.swd(gx[:m], rx[:m], dirs)
    ref_s = time.perf_counter() - t0
    res["float64_restatement"] = dict(images_a_side=m, seconds=ref_s, scaled_to_one_evaluation_s=ref_s * samples / m * 2,
                                      scaled_to_the_first_evaluation_s=ref_s * samples / m * 4, pooled_value=want.tolist())
    return res


def separation(per_class=100, n_dir=128, classes=4):
    from rcgan_amd import swd as SW
    from tests import swd_ref as SR
    labels = np.random.RandomState(5).permutation(np.repeat(np.arange(classes), per_class))
    real_labels = np.random.RandomState(6).permutation(np.repeat(np.arange(classes), 2 * per_class))
    rs = np.random.RandomState(7)
    draw = templates(32, labels)
    one = templates(33, np.arange(classes))
    collapsed = np.clip(np.rint(one[labels].astype(np.float64) + 2.0 * rs.randn(len(labels), 32, 32, 3)), 0, 255).astype(np.uint8)
    blurred = np.clip(np.rint(SR.up(SR.down(draw))), 0, 255).astype(np.uint8)
    ev = SW.SwdEvaluator(classes, directions=n_dir)
    ev.prepare_real(templates(31, real_labels), real_labels)
    out = dict(classes=classes, images_per_class=per_class, directions=n_dir)
    for name, (x, y) in dict(second_draw=(draw, labels), labels_shuffled=(draw, rs.permutation(labels)), collapsed=(collapsed, labels),
                             blurred=(blurred, labels)).items():
        r = ev.evaluate(x, y)
        out[name] = dict(pooled_levels=[float(v) for v in r["swd_levels"]], intra_class_levels=[float(v) for v in r["intra_class_swd_levels"]],
                         intra_class_swd=r["intra_class_swd"], intra_class_swd_se=r["intra_class_swd_se"])
        out["floor"] = dict(pooled_levels=[float(v) for v in r["floor_swd_levels"]], intra_class_levels=[float(v) for v in r["floor_intra_class_swd_levels"]],
                            intra_class_swd=r["floor_intra_class_swd"])
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-images", type=int, default=500)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its bench.py is timed next to this tree's")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swd.json"))
    a = ap.parse_args()
    from rcgan_amd import _lib as L
    from rcgan_amd.runtime import Context
    out = {"kernel_source_hash": L.source_hash()}
    ctx = Context(0, "f32", arena_bytes=1 << 20, ws_bytes=1 << 20)
    labels = np.sort(np.arange(a.samples) % K)
    images = templates(1, labels)
    out["calls_pooled"] = calls(ctx, images, [a.samples])
    out["calls_10_classes"] = calls(ctx, images, np.bincount(labels, minlength=K).tolist())
    out["calls_pooled_level_2"] = calls(ctx, images, [a.samples], level=2)
    ctx.close()
    print("calls timed", file=sys.stderr, flush=True)
    out["evaluation"] = evaluation(a.samples, a.repeats, a.ref_images)
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
