#!/usr/bin/env python3
"""D.Block.2 of the CIFAR critic, forward: one fused launch (rcgan_dblock2_fwd) vs the four launches it replaces (2x2 mean, 1x1 shortcut,
register-filter Conv1, Conv2 + pool as one 4x4 stride-2 convolution), in one process, HIP events on the launch stream.  After a warm-up
the two routes alternate in trains of about 0.3 s, five repetitions each; the bar is mean(four) - mean(fused) > 3 x the larger of the
two routes' ranges (slowest minus fastest train).  STAMPS=1: the fused kernel's per-workgroup s_memtime segments.
Then the same for the data gradient: rcgan_dblock2_bwd vs the four backward launches (Conv2 + pool's data gradient in its sub-pixel form,
the register-filter Conv1 data gradient, the 1x1 shortcut's, the pool's adjoint accumulated into dx); its bar is mean(four) - mean(fused) >
the two routes' ranges added together.
usage: python scripts/bench_dblock2.py [n] [--json FILE]"""
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
    ctx = Context(0, "bf16", arena_bytes=1 << 30, ws_bytes=1 << 30)
    lib, h = ctx.lib, ctx.h
    P = C.c_void_p
    x = ctx.empty((n, 16, 16, 128))
    ctx.check(lib.rcgan_rng_fill(h, x.size, x.dtype, 1, 0.0, 1.0, 7, None, P(x.ptr)))
    d1 = L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, L.BF16, L.CONV_IN_RELU)
    d2 = L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, L.BF16, L.CONV_IN_RELU | L.CONV_OUT_MEANPOOL2 | L.CONV_ACCUMULATE)
    ds = L.ConvDesc(n, 8, 8, 128, 128, 1, 1, 1, L.BF16, 0)
    prep, bias = {}, {}
    for i, (k, d, shape) in enumerate((("s", ds, (1, 1, 128, 128)), ("1", d1, (3, 3, 128, 128)), ("2", d2, (3, 3, 128, 128)))):
        w = ctx.empty(shape, L.F32)
        ctx.check(lib.rcgan_rng_fill(h, w.size, L.F32, 1, 0.0, 0.03, 9 + i, None, P(w.ptr)))
        prep[k] = ctx.arena.alloc(lib.rcgan_conv_prepared_bytes(C.byref(d)))
        ctx.check(lib.rcgan_conv_prepare(h, C.byref(d), P(w.ptr), None, P(prep[k])))
        bias[k] = ctx.empty((128,), L.F32)
        ctx.check(lib.rcgan_rng_fill(h, 128, L.F32, 1, 0.0, 0.1, 19 + i, None, P(bias[k].ptr)))
    frag1 = ctx.arena.alloc(lib.rcgan_conv_rf_fragment_bytes(C.byref(d1)))
    fragb = ctx.arena.alloc(lib.rcgan_dblock2_fragment_bytes())
    one = lambda v: (C.c_void_p * 1)(v)
    ctx.check(lib.rcgan_fragments_prepare_dblock2(h, None, None, 1, C.byref(d1), one(prep["1"]), one(frag1), P(prep["2"]), P(prep["s"]), P(fragb)))
    hh, xp, y = ctx.empty((n, 16, 16, 128)), ctx.empty((n, 8, 8, 128)), ctx.empty((n, 8, 8, 128))
    assert lib.rcgan_dblock2_ok(C.byref(d1), P(frag1), P(fragb))

    def fused():
        ctx.check(lib.rcgan_dblock2_fwd(h, C.byref(d1), P(x.ptr), P(frag1), P(fragb), P(bias["1"].ptr), P(bias["2"].ptr), P(bias["s"].ptr),
                                        P(hh.ptr), P(xp.ptr), P(y.ptr)))

    def four():
        ctx.check(lib.rcgan_meanpool2_fwd(h, n, 16, 16, 128, L.BF16, P(x.ptr), P(xp.ptr)))
        ctx.check(lib.rcgan_conv2d_fwd(h, C.byref(ds), P(xp.ptr), P(prep["s"]), P(bias["s"].ptr), P(y.ptr)))
        ctx.check(lib.rcgan_conv2d_rf(h, C.byref(d1), 0, P(x.ptr), P(frag1), P(bias["1"].ptr), None, None, P(hh.ptr)))
        ctx.check(lib.rcgan_conv2d_fwd(h, C.byref(d2), P(hh.ptr), P(prep["2"]), P(bias["2"].ptr), P(y.ptr)))

    # ---- the data gradient: dy, and the forward's h and x as masks ----
    dy, dh, dx, dxp = ctx.empty((n, 8, 8, 128)), ctx.empty((n, 16, 16, 128)), ctx.empty((n, 16, 16, 128)), ctx.empty((n, 8, 8, 128))
    ctx.check(lib.rcgan_rng_fill(h, dy.size, dy.dtype, 1, 0.0, 1.0, 29, None, P(dy.ptr)))
    d2b = L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, L.BF16, L.CONV_IN_RELU | L.CONV_OUT_MEANPOOL2)
    ws = C.c_void_p(ctx.ws_ptr)

    def fused_bwd():
        ctx.check(lib.rcgan_dblock2_bwd(h, C.byref(d1), P(dy.ptr), P(hh.ptr), P(x.ptr), P(frag1), P(fragb), P(dh.ptr), P(dx.ptr)))

    def four_bwd():
        ctx.check(lib.rcgan_conv2d_bwd_data(h, C.byref(d2b), P(dy.ptr), P(prep["2"]), P(hh.ptr), P(dh.ptr), ws, ctx.ws_bytes))
        ctx.check(lib.rcgan_conv2d_rf(h, C.byref(d1), 1, P(dh.ptr), P(frag1), None, P(x.ptr), None, P(dx.ptr)))
        ctx.check(lib.rcgan_conv2d_bwd_data(h, C.byref(ds), P(dy.ptr), P(prep["s"]), None, P(dxp.ptr), ws, ctx.ws_bytes))
        ctx.check(lib.rcgan_meanpool2_bwd(h, n, 16, 16, 128, L.BF16, P(dxp.ptr), P(dx.ptr), 1))

    result = {"n": n}
    if os.environ.get("STAMPS"):
        import torch
        st = torch.zeros(2 * n * 16, dtype=torch.int64, device=ctx.device)
        fused(); fused()
        ctx.check(lib.rcgan_debug_stamps(h, P(st.data_ptr())))
        fused()
        ctx.sync()
        ctx.check(lib.rcgan_debug_stamps(h, None))
        t = st.cpu().numpy().reshape(2 * n, 16).astype(np.float64) / 2270.0          # us @ 2.27 GHz (scripts/bench_trunk.py)
        seg = {"patch wait": t[:, 2] - t[:, 0],
               "stage 1 K loop": (t[:, 3] - t[:, 2]) + (t[:, 5] - t[:, 4]) + (t[:, 7] - t[:, 6]),
               "exchange and epilogue": (t[:, 4] - t[:, 3]) + (t[:, 6] - t[:, 5]) + (t[:, 8] - t[:, 7]),
               "stage 2 K loop": t[:, 9] - t[:, 8], "epilogue": t[:, 10] - t[:, 9], "total": t[:, 10] - t[:, 0]}
        print("per-workgroup segments, us (mean over %d workgroups):" % (2 * n))
        for k, v in seg.items():
            print("  %-22s %6.2f" % (k, v.mean()))
        result["stamps_us"] = {k: round(float(v.mean()), 3) for k, v in seg.items()}
        fused()                                     # (h for the masks)
        st.zero_()
        fused_bwd(); fused_bwd()
        ctx.check(lib.rcgan_debug_stamps(h, P(st.data_ptr())))
        fused_bwd()
        ctx.sync()
        ctx.check(lib.rcgan_debug_stamps(h, None))
        t = st.cpu().numpy().reshape(2 * n, 16).astype(np.float64) / 2270.0
        seg = {"dy and h wait": t[:, 2] - t[:, 0], "shortcut": t[:, 3] - t[:, 2], "stage 1: four classes": t[:, 7] - t[:, 3],
               "filters of stage 2, barrier": t[:, 8] - t[:, 7],
               "stage 2 K loop": (t[:, 9] - t[:, 8]) + (t[:, 11] - t[:, 10]),
               "exchange and epilogue": (t[:, 10] - t[:, 9]) + (t[:, 12] - t[:, 11]), "total": t[:, 12] - t[:, 0]}
        print("data gradient, per-workgroup segments, us (mean over %d workgroups):" % (2 * n))
        for k, v in seg.items():
            print("  %-28s %6.2f" % (k, v.mean()))
        result["bwd_stamps_us"] = {k: round(float(v.mean()), 3) for k, v in seg.items()}

    def train(fn, reps):
        ctx.event_record(0)
        for _ in range(reps):
            fn()
        ctx.event_record(1)
        return ctx.event_elapsed_ms(0, 1) * 1e3 / reps

    for fn in (fused, four):
        for _ in range(20):
            fn()
    reps = {fn: max(50, int(0.3e6 / train(fn, 200))) for fn in (fused, four)}
    us = {fused: [], four: []}
    for _ in range(5):
        for fn in (fused, four):
            us[fn].append(train(fn, reps[fn]))
    for name, fn in (("fused", fused), ("four launches", four)):
        v = us[fn]
        print("n=%d %-14s mean %7.2f us  range %.2f  (%s)" % (n, name, np.mean(v), max(v) - min(v), " ".join("%.2f" % t for t in v)))
        result[name.replace(" ", "_") + "_us"] = [round(t, 3) for t in v]
    gain = float(np.mean(us[four]) - np.mean(us[fused]))
    noise = float(max(max(v) - min(v) for v in us.values()))
    result.update(gain_us=round(gain, 3), largest_range_us=round(noise, 3), bar_met=bool(gain > 3 * noise))
    print("four - fused = %.2f us; 3 x largest range = %.2f us: bar %s" % (gain, 3 * noise, "met" if gain > 3 * noise else "NOT met"))
    # ---- the data gradient, same method ----
    fused()
    for fn in (fused_bwd, four_bwd):
        for _ in range(20):
            fn()
    reps = {fn: max(50, int(0.3e6 / train(fn, 200))) for fn in (fused_bwd, four_bwd)}
    us = {fused_bwd: [], four_bwd: []}
    for _ in range(5):
        for fn in (fused_bwd, four_bwd):
            us[fn].append(train(fn, reps[fn]))
    for name, fn in (("fused bwd", fused_bwd), ("four bwd launches", four_bwd)):
        v = us[fn]
        print("n=%d %-18s mean %7.2f us  range %.2f  (%s)" % (n, name, np.mean(v), max(v) - min(v), " ".join("%.2f" % t for t in v)))
        result[name.replace(" ", "_") + "_us"] = [round(t, 3) for t in v]
    gain = float(np.mean(us[four_bwd]) - np.mean(us[fused_bwd]))
    noise = float(sum(max(v) - min(v) for v in us.values()))
    result.update(bwd_gain_us=round(gain, 3), bwd_ranges_added_us=round(noise, 3), bwd_bar_met=bool(gain > noise))
    print("four bwd - fused bwd = %.2f us; the two ranges added = %.2f us: bar %s" % (gain, noise, "met" if gain > noise else "NOT met"))
    if out_json:
        with open(out_json, "w") as f:
            json.dump(result, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
