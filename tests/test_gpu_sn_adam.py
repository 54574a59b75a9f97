"""rcgan_sn_bwd_adam (csrc/sn.hip: the spectral-norm backward with TF-Adam inside its second launch, rider workgroups for the rest of
the optimiser group's slab) against float64, at the shapes and slab layouts where its branches differ:
  * dW (still written to the gradient slab) against oracle.nn.spectral_norm_bwd;
  * w / m / v over the WHOLE slab against oracle.nn.adam_tf applied to the GPU's own dW (and to the uploaded gradient of the
    parameters between the spectrally normalised weights), t = t0 + 1 -- the Adam arithmetic separated from the backward;
  * the same inputs through rcgan_sn_bwd + rcgan_adam_tf: dW bit for bit, w / m / v to 2 ulp.
Also: graph replay with a new learning rate, the host-side argument checks, and ops.spectral_norm_batch's fall-back to the separate
optimiser launch when a group has more gaps than one fused call takes."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nn
from tests.gpu_util import assert_close, make_ctx

pytestmark = pytest.mark.gpu

LR, BETA2, EPS = 1e-3, 0.9, 1e-8


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32")
    yield c
    c.close()


def _put(ctx, t, arr):
    with torch.cuda.stream(ctx.stream):
        t.copy_(torch.from_numpy(np.ascontiguousarray(arr, np.float32)))


def _get(ctx, t):
    with torch.cuda.stream(ctx.stream):
        out = t.detach().cpu()
    ctx.stream.synchronize()
    return out.numpy().astype(np.float64)


class Slab:
    """A ParamGroup(sn_scratch=True) laid out from ``layout``: ("sn", k, c[, prior]) is a spectrally normalised weight [k, c] (prior:
    its gradient already holds a nonzero dW that the backward accumulates onto), ("p", n) a plain parameter of n floats (a bias or
    embedding: the rider workgroups update it, together with the group's alignment holes).  Random initial w, m, v, u, dW_bar and
    gradients of everything outside the weights."""

    def __init__(self, ctx, layout, seed):
        from rcgan_amd import _lib as L
        from rcgan_amd.runtime import ParamGroup
        rs = np.random.RandomState(seed)
        specs, self.sn = [], []
        for i, e in enumerate(layout):
            if e[0] == "sn":
                name = "w%d" % i
                specs.append((name, (e[1], e[2]), (0.1 * rs.randn(e[1], e[2])).astype(np.float32)))
                self.sn.append((name, e[1], e[2], len(e) > 3 and e[3]))
            else:
                specs.append(("b%d" % i, (e[1],), rs.randn(e[1]).astype(np.float32)))
        self.pg = pg = ParamGroup(ctx, specs, sn_scratch=True)
        n = pg.count
        self.w0 = _get(ctx, pg.value).astype(np.float32)
        self.m0 = (0.01 * rs.randn(n)).astype(np.float32)
        self.v0 = rs.uniform(1e-6, 1e-3, n).astype(np.float32)
        self.g0 = rs.randn(n).astype(np.float32)          # the gradient of everything outside the weights ...
        self.u0, self.dwbar, self.u = {}, {}, {}
        for name, k, c, prior in self.sn:
            o = pg.offsets[name]
            self.g0[o:o + k * c] = rs.randn(k * c) if prior else 0.0       # ... and what the weights' gradient holds before the call
            self.u0[name] = rs.randn(c).astype(np.float32)
            self.dwbar[name] = rs.randn(k, c).astype(np.float32)
            self.u[name] = ctx.persistent((c,), L.F32)
        cover = sorted((pg.offsets[s[0]], pg.offsets[s[0]] + s[1] * s[2]) for s in self.sn)
        self.ranges, at = [], 0
        for lo, hi in cover:
            if lo > at:
                self.ranges.append((at, lo))
            at = hi
        if at < n:
            self.ranges.append((at, n))

    def reset(self, ctx, t0):
        """Initial w / m / v / gradient / u on the device, {LR, t0} as the group's device hyper-parameters."""
        from rcgan_amd import _lib as L
        pg = self.pg
        for t, a in ((pg.value, self.w0), (pg.m, self.m0), (pg.v, self.v0)):
            _put(ctx, t, a)
        for name, *_ in self.sn:
            ctx.upload(self.u0[name], L.F32, out=self.u[name])
        pg.set_hyper_device(LR, t0)

    def items(self, name):
        o = self.pg.offsets[name]
        return o, o + self.pg.shapes[name][0] * self.pg.shapes[name][1]

    def dw_ref(self, name, w=None):
        """float64 dW of weight ``name`` from dW_bar, through the power iteration run on the initial W and u (w: the W the backward
        reads, when it differs from the one the forward saw -- a replayed backward after an update)."""
        lo, hi = self.items(name)
        k, c = self.pg.shapes[name]
        w0 = self.w0[lo:hi].reshape(k, c).astype(np.float64)
        u = self.u0[name].astype(np.float64)[None]
        cache = nn.spectral_norm_fwd(w0, u)[3]
        return nn.spectral_norm_bwd(self.dwbar[name].astype(np.float64), w0 if w is None else w.reshape(k, c), u, cache).reshape(-1)


def _adam_ref(w, g, m, v, t, lr, beta1, clip, grad_scale):
    f = lambda a: np.asarray(a, np.float64)
    return nn.adam_tf(f(w), f(g) * grad_scale, f(m), f(v), t, lr, beta1, BETA2, EPS, clip=clip if clip > 0 else None)


def _ulp_close(a, b, n, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = n * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    bad = np.abs(a - b) > tol
    assert not bad.any(), "%s: %d elements beyond %d ulp, first at %d (%r vs %r)" % (
        what, int(bad.sum()), n, int(np.argmax(bad)), float(a[bad][0]), float(b[bad][0]))


def _ops_step(ctx, sl, t0, hp, fused):
    """Forward (ops.spectral_norm_batch) + backward through ops with ctx.sn_adam set (fused) or not (then rcgan_adam_tf on the whole
    slab with {lr, t0 + 1} from device memory).  Returns the slabs after the step, the device t and whether the fused call ran."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    pg = sl.pg
    sl.reset(ctx, t0)
    ctx.new_step()
    pg.zero_grad()
    _put(ctx, pg.grad, sl.g0)
    params = []
    for name, *_ in sl.sn:
        p = pg.param(name)
        p.req = True
        params.append((p, sl.u[name], True))
    Ws = O.spectral_norm_batch(ctx, params)
    for (name, *_), W in zip(sl.sn, Ws):
        assert W.dwbar is not None and W.dwbar.base is pg.gradbuf      # the group's d/dW_bar slab
        ctx.upload(sl.dwbar[name], L.F32, out=W.dwbar)
    ctx.sn_adam = dict(group=pg, beta1=hp["beta1"], beta2=BETA2, grad_scale=hp["grad_scale"], clip=hp["clip"]) if fused else None
    try:
        ctx.backward()
        done = bool(ctx.sn_adam and ctx.sn_adam.get("done"))
    finally:
        ctx.sn_adam = None
    if not fused:
        pg.set_hyper_device(LR, t0 + 1)
        pg.adam_captured(hp["beta1"], BETA2, EPS, clip=hp["clip"], grad_scale=hp["grad_scale"])
    ctx.sync()
    out = {k: _get(ctx, getattr(pg, k)) for k in ("value", "m", "v", "grad")}
    out["t"] = float(_get(ctx, pg.hyper)[1])
    out["done"] = done
    return out


def _check_against_fp64(sl, out, t0, hp, what=""):
    """dW of every weight against spectral_norm_bwd (5e-5 of max|ref|, as test_spectral_norm); w / m / v of the whole slab against ONE
    float64 Adam update of the GPU's own gradient slab (2e-6 of max|ref|, as test_adam_tf); the device step count exactly."""
    for name, k, c, prior in sl.sn:
        lo, hi = sl.items(name)
        ref = sl.dw_ref(name) + (sl.g0[lo:hi] if prior else 0.0)
        assert_close(out["grad"][lo:hi], ref, 5e-5, "%s dW of %s [%d,%d]" % (what, name, k, c))
    for lo, hi in sl.ranges:            # the gradient outside the weights is read, never written
        assert np.array_equal(out["grad"][lo:hi], sl.g0[lo:hi]), (what, lo, hi)
    w, m, v = _adam_ref(sl.w0, out["grad"], sl.m0, sl.v0, t0 + 1, LR, hp["beta1"], hp["clip"], hp["grad_scale"])
    assert_close(out["value"], w, 2e-6, what + " w")
    assert_close(out["m"], m, 2e-6, what + " m")
    assert_close(out["v"], v, 2e-6, what + " v")
    assert out["t"] == t0 + 1, (what, out["t"], t0)
    if hp["clip"] > 0:
        assert np.abs(out["value"]).max() == np.float32(hp["clip"]), "the clip case clamps no weight"


def _pairs(n):
    return [x for _ in range(n) for x in (("sn", 3, 128), ("p", 3))]


# (layout, expected number of ranges, hyper-parameters, t0).  c = 128: the prefetch path; 256, 1024: float4 beyond 128 columns; 3, 10,
# 12: the scalar path -- each with a k that is not a multiple of 32 (a partial last chunk).  More than SN_BATCH = 24 weights: several
# launch pairs, riders and ranges in the last one only, t advanced once.
H0 = dict(beta1=0.0, clip=0.0, grad_scale=1.0)
CASES = {
    "one_item": ([("sn", 1, 128)], 0, H0, 0),
    "items_tile_the_slab": ([("sn", 1, 128), ("sn", 31, 256, True)], 0, dict(beta1=0.5, clip=0.0, grad_scale=0.25), 7),
    "range_at_offset_0": ([("p", 5), ("sn", 33, 128, True)], 1, dict(beta1=0.5, clip=0.0, grad_scale=0.25), 7),
    "range_at_the_end": ([("sn", 300, 10), ("p", 7)], 1, dict(beta1=0.0, clip=0.15, grad_scale=1.0), 0),
    "odd_ranges_1_7_130": ([("sn", 21, 3), ("sn", 19, 3, True), ("sn", 19, 10), ("p", 128), ("sn", 33, 3), ("sn", 1, 3)], 5,
                           dict(beta1=0.5, clip=0.15, grad_scale=0.25), 7),
    "c1024": ([("sn", 33, 1024), ("p", 1)], 1, dict(beta1=0.0, clip=0.0, grad_scale=0.25), 7),
    "sn_max_k": ([("sn", 4096, 10), ("p", 2), ("sn", 4096, 128)], 1, H0, 7),
    "24_items": ([("sn", 33 if i % 4 == 0 else 32, 128) if i % 2 == 0 else ("sn", 31, 256, i == 3) for i in range(24)], 0,
                 dict(beta1=0.5, clip=0.0, grad_scale=1.0), 0),
    "25_items": ([("p", 3)] + [("sn", 33, 128, True)] * 12 + [("p", 130)] + [("sn", 19, 12)] * 13, 15,
                 dict(beta1=0.0, clip=0.15, grad_scale=0.25), 7),
    "50_items": ([("sn", 3, 128)] * 20 + [("p", 7)] + [("sn", 1, 1024)] * 20 + [("p", 1)] + [("sn", 33, 10, True)] * 10 + [("p", 64)],
                 12, dict(beta1=0.5, clip=0.0, grad_scale=0.25), 0),
    "48_ranges": (_pairs(48), 48, H0, 7),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_sn_backward_adam_against_fp64(ctx, case):
    layout, n_ranges, hp, t0 = CASES[case]
    sl = Slab(ctx, layout, seed=sum(map(ord, case)))
    assert len(sl.ranges) == n_ranges, sl.ranges
    if case == "range_at_offset_0":
        assert sl.ranges[0][0] == 0
    if case == "range_at_the_end":
        assert sl.ranges[-1][1] == sl.pg.count
    if case == "odd_ranges_1_7_130":
        assert {1, 7, 130} <= {hi - lo for lo, hi in sl.ranges}
    fused = _ops_step(ctx, sl, t0, hp, fused=True)
    assert fused["done"], "ops.spectral_norm_batch did not take the fused call"
    _check_against_fp64(sl, fused, t0, hp, case)
    # the same inputs through the two-launch backward + the separate optimiser launch
    sep = _ops_step(ctx, sl, t0, hp, fused=False)
    assert not sep["done"]
    assert np.array_equal(fused["grad"], sep["grad"]), case + ": dW differs from rcgan_sn_bwd"
    for k in ("value", "m", "v"):
        _ulp_close(fused[k], sep[k], 2, "%s %s: fused vs rcgan_adam_tf" % (case, k))
    assert sep["t"] == fused["t"]


# ---------------------------------------------------------------------------------------------------- the C ABI directly
class Abi:
    """The forward (rcgan_sn_power_iter) with save buffers of our own, so that rcgan_sn_bwd_adam can be called with explicit items and
    ranges: accumulate = 0 items, graph capture of the single call, argument checks."""

    def __init__(self, ctx, sl, accumulate):
        from rcgan_amd import _lib as L
        self.ctx, self.sl = ctx, sl
        n = len(sl.sn)
        self.saves, self.sigmas, self.dwb = [], [], []
        for name, k, c, _ in sl.sn:
            self.saves.append(ctx.persistent((ctx.lib.rcgan_sn_save_floats(k, c),), L.F32))
            self.sigmas.append(ctx.persistent((1,), L.F32))
            self.dwb.append(ctx.upload(sl.dwbar[name], L.F32, out=ctx.persistent((k, c), L.F32)))
        self.acc = accumulate
        pg = sl.pg
        self.fwd = (L.SnItem * n)(*[L.SnItem(pg.value.data_ptr() + 4 * pg.offsets[name], sl.u[name].ptr, sg.ptr, sv.ptr, k, c, 1)
                                    for (name, k, c, _), sg, sv in zip(sl.sn, self.sigmas, self.saves)])
        self.bwd = (L.SnBwdItem * n)(*[L.SnBwdItem(pg.value.data_ptr() + 4 * pg.offsets[name], d.ptr, pg.grad.data_ptr() + 4 * pg.offsets[name],
                                                   sv.ptr, k, c, a)
                                       for (name, k, c, _), d, sv, a in zip(sl.sn, self.dwb, self.saves, accumulate)])

    def forward(self, t0):
        ctx, pg = self.ctx, self.sl.pg
        self.sl.reset(ctx, t0)
        _put(ctx, pg.grad, self.sl.g0)
        ctx.check(ctx.lib.rcgan_sn_power_iter(ctx.h, self.fwd, len(self.fwd)))

    def call(self, hp, items=None, ranges=None):
        """rcgan_sn_bwd_adam on the group's slabs (default: this object's items and the slab's own ranges); returns its status."""
        from rcgan_amd import _lib as L
        ctx, pg = self.ctx, self.sl.pg
        items = self.bwd if items is None else items
        flat = [x for r in (self.sl.ranges if ranges is None else ranges) for x in r]
        ra = (C.c_size_t * max(len(flat), 1))(*flat)
        opt = L.SnAdam(pg.value.data_ptr(), pg.grad.data_ptr(), pg.m.data_ptr(), pg.v.data_ptr(), pg.count, pg.hyper.data_ptr(),
                       hp["beta1"], BETA2, EPS, hp["clip"], hp["grad_scale"], len(flat) // 2, ra)
        return ctx.lib.rcgan_sn_bwd_adam(ctx.h, items, len(items), C.byref(opt))

    def result(self):
        ctx, pg = self.ctx, self.sl.pg
        ctx.sync()
        out = {k: _get(ctx, getattr(pg, k)) for k in ("value", "m", "v", "grad")}
        out["t"] = float(_get(ctx, pg.hyper)[1])
        return out


ABI_LAYOUT = [("p", 9), ("sn", 33, 128), ("sn", 19, 10), ("p", 1), ("sn", 31, 256), ("sn", 1, 3)]
ABI_HP = dict(beta1=0.5, clip=0.0, grad_scale=0.25)


def _check_abi_dw(ab, out, w_before=None, what=""):
    """dW of every item against float64, for items that overwrite (accumulate = 0) or accumulate onto the initial gradient; w_before:
    the weights the call read (after earlier replays)."""
    sl = ab.sl
    for (name, k, c, _), acc in zip(sl.sn, ab.acc):
        lo, hi = sl.items(name)
        ref = sl.dw_ref(name, None if w_before is None else w_before[lo:hi]) + (sl.g0[lo:hi] if acc else 0.0)
        assert_close(out["grad"][lo:hi], ref, 5e-5, "%s dW of %s" % (what, name))


def test_fused_call_through_the_abi_overwrite_and_accumulate(ctx):
    """accumulate = 0 next to accumulate = 1 on a nonzero gradient (ops always accumulates), against float64."""
    sl = Slab(ctx, [(e[0], e[1], e[2], True) if e[0] == "sn" else e for e in ABI_LAYOUT], seed=11)
    ab = Abi(ctx, sl, accumulate=[0, 1, 0, 1])
    ab.forward(t0=3)
    ctx.check(ab.call(ABI_HP))
    out = ab.result()
    _check_abi_dw(ab, out, what="abi")
    w, m, v = _adam_ref(sl.w0, out["grad"], sl.m0, sl.v0, 4, LR, ABI_HP["beta1"], ABI_HP["clip"], ABI_HP["grad_scale"])
    assert_close(out["value"], w, 2e-6, "abi w")
    assert_close(out["m"], m, 2e-6, "abi m")
    assert_close(out["v"], v, 2e-6, "abi v")
    assert out["t"] == 4


def test_fused_call_replayed_from_a_graph_with_a_new_learning_rate(ctx):
    """One rcgan_sn_bwd_adam call captured, replayed twice with lr rewritten by set_hyper_device in between: each replay is one Adam
    update with the step count it advanced itself and the lr of the moment.  (accumulate = 0: each replay's dW is that of the W it
    reads -- the updated one -- through the power iteration the forward saved.)"""
    sl = Slab(ctx, ABI_LAYOUT, seed=12)
    ab = Abi(ctx, sl, accumulate=[0, 0, 0, 0])
    t0 = 7
    ab.forward(t0)
    ctx.sync()
    ctx.graph_begin()
    try:
        ctx.check(ab.call(ABI_HP))
    except BaseException:
        ctx.graph_abort()
        raise
    gid = ctx.graph_end()
    try:
        prev = dict(value=sl.w0.astype(np.float64), m=sl.m0.astype(np.float64), v=sl.v0.astype(np.float64))
        for r, lr in enumerate((LR, 0.5 * LR)):
            sl.pg.set_hyper_device(lr, t0 + r)
            ctx.graph_launch(gid)
            out = ab.result()
            _check_abi_dw(ab, out, w_before=None if r == 0 else prev["value"], what="replay %d" % r)
            w, m, v = _adam_ref(prev["value"], out["grad"], prev["m"], prev["v"], t0 + r + 1, lr, ABI_HP["beta1"], ABI_HP["clip"],
                                ABI_HP["grad_scale"])
            assert_close(out["value"], w, 2e-6, "replay %d w" % r)
            assert_close(out["m"], m, 2e-6, "replay %d m" % r)
            assert_close(out["v"], v, 2e-6, "replay %d v" % r)
            assert out["t"] == t0 + r + 1
            prev = out
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))


def test_fused_call_rejects_what_it_cannot_take(ctx):
    """Host-side argument checks, all of them before any launch: RCGAN_EINVALID_ARG and nothing written.  Then a valid call on the same
    context is still right."""
    from rcgan_amd import _lib as L
    sl = Slab(ctx, ABI_LAYOUT, seed=13)
    ab = Abi(ctx, sl, accumulate=[1, 1, 1, 1])
    ab.forward(t0=0)
    ctx.sync()
    before = ab.result()
    pg = sl.pg
    rs = sl.ranges
    assert len(rs) == 3 and rs[0] == (0, 64)
    many = [(i, i + 1) for i in range(L.SN_MAX_RANGES + 1)]          # one range more than a call takes
    w1 = pg.value.data_ptr() + 4 * pg.offsets["w1"]
    moved = (L.SnBwdItem * 1)(L.SnBwdItem(w1, ab.dwb[0].ptr, pg.grad.data_ptr() + 4 * (pg.offsets["w1"] + 64), ab.saves[0].ptr, 33, 128, 1))
    bad = {
        "49 ranges": dict(ranges=many),
        "a gap": dict(ranges=[rs[0], rs[1]]),                                             # the tail range left out
        "an overlap": dict(ranges=[rs[0], (rs[1][0] - 1, rs[1][1]), rs[2]]),
        "dw and w at different slab offsets": dict(items=moved, ranges=[(0, pg.offsets["w1"]), (pg.offsets["w1"] + 33 * 128, pg.count)]),
    }
    # a vector-path item (c % 4 == 0) at a slab offset that is not a multiple of 4 floats: [2, 34) of a 64-float slab (the tiling is right)
    sl4 = Slab(ctx, [("sn", 8, 4)], seed=14)
    ab4 = Abi(ctx, sl4, accumulate=[1])
    ab4.forward(t0=0)
    p4 = sl4.pg
    off2 = (L.SnBwdItem * 1)(L.SnBwdItem(p4.value.data_ptr() + 8, ab4.dwb[0].ptr, p4.grad.data_ptr() + 8, ab4.saves[0].ptr, 8, 4, 1))
    odd_dwbar = (L.SnBwdItem * 1)(L.SnBwdItem(p4.value.data_ptr(), ab4.dwb[0].ptr + 4, p4.grad.data_ptr(), ab4.saves[0].ptr, 8, 4, 1))
    for what, kw in bad.items():
        rc = ab.call(ABI_HP, **kw)
        assert rc == L.EINVALID_ARG, (what, rc, ctx.lib.rcgan_last_error(ctx.h))
    for what, items, ranges in (("slab offset 2 floats", off2, [(0, 2), (34, 64)]), ("misaligned dW_bar", odd_dwbar, [(32, 64)])):
        rc = ab4.call(ABI_HP, items=items, ranges=ranges)
        assert rc == L.EINVALID_ARG, (what, rc, ctx.lib.rcgan_last_error(ctx.h))
        assert b"16-byte" in ctx.lib.rcgan_last_error(ctx.h), what
    after = ab.result()
    for k in ("value", "m", "v", "grad"):
        assert np.array_equal(after[k], before[k]), "a rejected call wrote %s" % k
    assert after["t"] == 0
    ctx.check(ab.call(ABI_HP))
    out = ab.result()
    _check_abi_dw(ab, out, what="after the rejections")
    w, m, v = _adam_ref(sl.w0, out["grad"], sl.m0, sl.v0, 1, LR, ABI_HP["beta1"], ABI_HP["clip"], ABI_HP["grad_scale"])
    assert_close(out["value"], w, 2e-6, "w after the rejections")
    assert out["t"] == 1


# ---------------------------------------------------------------------------------------------------- ops: fused or not
@pytest.mark.parametrize("pairs", [48, 50])
def test_ops_falls_back_beyond_the_fused_call_s_range_limit(ctx, pairs):
    """A group of ``pairs`` weights each followed by a bias: that many gaps.  Up to SN_MAX_RANGES the fused call takes the step;
    beyond it ops.spectral_norm_batch runs the plain backward (sn_adam["done"] stays False) and the caller's separate optimiser launch
    gives the same float64 update."""
    from rcgan_amd import _lib as L
    sl = Slab(ctx, _pairs(pairs), seed=pairs)
    assert len(sl.ranges) == pairs
    hp = dict(beta1=0.0, clip=0.0, grad_scale=0.5)
    out = _ops_step(ctx, sl, 5, hp, fused=True)
    assert out["done"] == (pairs <= L.SN_MAX_RANGES)
    if not out["done"]:
        # dW alone; the update is the caller's, as cifar.py's d_step does it when the step's last launch did not apply it
        for name, *_ in sl.sn:
            lo, hi = sl.items(name)
            assert_close(out["grad"][lo:hi], sl.dw_ref(name), 5e-5, "dW of " + name)
        assert np.array_equal(out["value"], sl.w0) and out["t"] == 5
        pg = sl.pg
        pg.set_hyper(LR, 6)
        pg.adam(hp["beta1"], BETA2, EPS, clip=hp["clip"], grad_scale=hp["grad_scale"])
        ctx.sync()
        out.update({k: _get(ctx, getattr(pg, k)) for k in ("value", "m", "v")})
        out["t"] = 6.0
    _check_against_fp64(sl, out, 5, hp, "%d gaps" % pairs)
