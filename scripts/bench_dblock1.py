#!/usr/bin/env python3
"""D.Block.1 of the CIFAR critic, forward: one fused launch (rcgan_dblock1_fwd) vs the three launches it replaces (the 1x1 shortcut and
the 3x3 Conv1 on the image-end kernel, Conv2 + pool as one 4x4 stride-2 convolution), in one process, HIP events on the launch stream.
After a warm-up the two routes alternate in trains of about 0.3 s, five repetitions each; the bar is mean(three) - mean(fused) > the two
routes' ranges (slowest minus fastest train) added together.  POOL=1: the generator step's pass -- the fused launch stores the pooled
images, the other side runs the meanpool2 launch as well.  STAMPS=1: the fused kernel's per-workgroup s_memtime segments.
usage: python scripts/bench_dblock1.py [n] [--json FILE]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import rcgan_amd  # noqa: E402,F401
from rcgan_amd import _lib as L  # noqa: E402
from rcgan_amd.runtime import Context  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 128
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    pool = bool(os.environ.get("POOL"))
    ctx = Context(0, "bf16", arena_bytes=1 << 30, ws_bytes=1 << 30)
    lib, h = ctx.lib, ctx.h
    P = C.c_void_p
    x = ctx.empty((n, 32, 32, 3))
    ctx.check(lib.rcgan_rng_fill(h, x.size, x.dtype, 1, 0.0, 1.0, 7, None, P(x.ptr)))
    d1 = L.ConvDesc(n, 32, 32, 3, 128, 3, 3, 1, L.BF16, 0)
    d2 = L.ConvDesc(n, 32, 32, 128, 128, 3, 3, 1, L.BF16, L.CONV_IN_RELU | L.CONV_OUT_MEANPOOL2 | L.CONV_ACCUMULATE)
    ds = L.ConvDesc(n, 16, 16, 3, 128, 1, 1, 1, L.BF16, 0)
    prep, bias = {}, {}
    for i, (k, d, shape) in enumerate((("s", ds, (1, 1, 3, 128)), ("1", d1, (3, 3, 3, 128)), ("2", d2, (3, 3, 128, 128)))):
        w = ctx.empty(shape, L.F32)
        ctx.check(lib.rcgan_rng_fill(h, w.size, L.F32, 1, 0.0, 0.03, 9 + i, None, P(w.ptr)))
        prep[k] = ctx.arena.alloc(lib.rcgan_conv_prepared_bytes(C.byref(d)))
        ctx.check(lib.rcgan_conv_prepare(h, C.byref(d), P(w.ptr), None, P(prep[k])))
        bias[k] = ctx.empty((128,), L.F32)
        ctx.check(lib.rcgan_rng_fill(h, 128, L.F32, 1, 0.0, 0.1, 19 + i, None, P(bias[k].ptr)))
    frag = ctx.arena.alloc(lib.rcgan_dblock1_fragment_bytes())
    ctx.check(lib.rcgan_fragments_prepare_dblocks(h, None, None, 0, None, None, None, None, None, None, P(prep["2"]), P(frag)))
    hh, xp, y = ctx.empty((n, 32, 32, 128)), ctx.empty((n, 16, 16, 3)), ctx.empty((n, 16, 16, 128))
    ctx.check(lib.rcgan_meanpool2_fwd(h, n, 32, 32, 3, L.BF16, P(x.ptr), P(xp.ptr)))
    assert lib.rcgan_dblock1_ok(C.byref(d1), P(frag))

    def fused():
        ctx.check(lib.rcgan_dblock1_fwd(h, C.byref(d1), P(x.ptr), P(prep["1"]), P(prep["s"]), P(frag), P(bias["1"].ptr), P(bias["2"].ptr),
                                        P(bias["s"].ptr), P(hh.ptr), P(xp.ptr) if pool else None, P(y.ptr)))

    def three():
        if pool:
            ctx.check(lib.rcgan_meanpool2_fwd(h, n, 32, 32, 3, L.BF16, P(x.ptr), P(xp.ptr)))
        ctx.check(lib.rcgan_conv2d_fwd(h, C.byref(ds), P(xp.ptr), P(prep["s"]), P(bias["s"].ptr), P(y.ptr)))
        ctx.check(lib.rcgan_conv2d_fwd(h, C.byref(d1), P(x.ptr), P(prep["1"]), P(bias["1"].ptr), P(hh.ptr)))
        ctx.check(lib.rcgan_conv2d_fwd(h, C.byref(d2), P(hh.ptr), P(prep["2"]), P(bias["2"].ptr), P(y.ptr)))

    result = {"n": n, "stores_pooled_images": pool}
    if os.environ.get("STAMPS"):
        import torch
        st = torch.zeros(4 * n * 16, dtype=torch.int64, device=ctx.device)
        fused(); fused()
        ctx.check(lib.rcgan_debug_stamps(h, P(st.data_ptr())))
        fused()
        ctx.sync()
        ctx.check(lib.rcgan_debug_stamps(h, None))
        t = st.cpu().numpy().reshape(4 * n, 16).astype(np.float64) / 2270.0          # us @ 2.27 GHz (scripts/bench_trunk.py)
        seg = {"patch wait": t[:, 1] - t[:, 0], "stage 1": t[:, 2] - t[:, 1], "h stores": t[:, 3] - t[:, 2],
               "stage 2 K loop": t[:, 4] - t[:, 3], "epilogue": t[:, 5] - t[:, 4], "total": t[:, 5] - t[:, 0]}
        print("per-workgroup segments, us (mean over %d workgroups):" % (4 * n))
        for k, v in seg.items():
            print("  %-22s %6.2f" % (k, v.mean()))
        result["stamps_us"] = {k: round(float(v.mean()), 3) for k, v in seg.items()}

    def train(fn, reps):
        ctx.event_record(0)
        for _ in range(reps):
            fn()
        ctx.event_record(1)
        return ctx.event_elapsed_ms(0, 1) * 1e3 / reps

    for fn in (fused, three):
        for _ in range(20):
            fn()
    reps = {fn: max(50, int(0.3e6 / train(fn, 200))) for fn in (fused, three)}
    us = {fused: [], three: []}
    for _ in range(5):
        for fn in (fused, three):
            us[fn].append(train(fn, reps[fn]))
    for name, fn in (("fused", fused), ("three launches", three)):
        v = us[fn]
        print("n=%d %-14s mean %7.2f us  range %.2f  (%s)" % (n, name, np.mean(v), max(v) - min(v), " ".join("%.2f" % t for t in v)))
        result[name.replace(" ", "_") + "_us"] = [round(t, 3) for t in v]
    gain = float(np.mean(us[three]) - np.mean(us[fused]))
    noise = float(sum(max(v) - min(v) for v in us.values()))
    result.update(gain_us=round(gain, 3), ranges_added_us=round(noise, 3), bar_met=bool(gain > noise))
    print("three - fused = %.2f us; the two ranges added = %.2f us: bar %s" % (gain, noise, "met" if gain > noise else "NOT met"))
    if out_json:
        with open(out_json, "w") as f:
            json.dump(result, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
