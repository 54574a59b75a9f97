"""rcgan_pair_diversity_fwd_bwd (csrc/diversity.hip) through ctypes, between guard bands (tests/guard.py), against the float64
restatement tests/diversity_ref.py.

The inputs lie on exact grids: images k/256 in [-1, 1], latents k/64 in [-4, 4] (all of them bf16, fp16 and fp32 numbers).  Every
difference, and every sum of up to 3072 of them, is then exact in fp32 in any order (|x differences| are multiples of 1/256 below 2:
a sum stays below 2^24 units; latent differences multiples of 1/64 below 8), and every sign is exact in every dtype.  What is left
is at most six fp32 roundings per number: two divisions by the row lengths, the ratio; for the gradient the products weight * scale
and P * D * dz and their quotient; for the loss weight / P, its product with the sum, P additions of terms and the accumulation.
Bounds:
    ratio_out            8 fp32 ulp; exactly -1 for a masked pair
    loss                 (P + 8) ulp of |old value| + (weight / P) sum|term|
    gradient             sign and zero pattern exact; magnitude 8 fp32 ulp (f32), relative 2^-8 (bf16), relative 2^-10 (fp16)
    accumulate = 1       one ulp of the stored dtype at the result (the old values are integers of magnitude 16 .. 31 and the fp32
                         steps stay below 2, so that 8 fp32 ulp of a step are at most half an fp32 ulp of the result; the other half
                         is the addition's rounding); masked and clamped pairs: the old bits
fp16 runs under a gradient scale of 1024, so that the step c_i is a normal fp16 number; the loss is unscaled, and one group of
cases reads half of the scale from device memory."""
import ctypes as C

import numpy as np
import pytest

from tests import diversity_ref as DR
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

PAIRS = (1, 3, 8)
ROWS = (3072, 2056, 24, 13)      # 16-byte route at its full length; chunks no multiple of the thread count; fewer chunks than threads;
LATENTS = (128, 5)               # the element-wise route
WEIGHT, L0 = 1.5, 1.25
ULP16 = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}       # spacing at 1


@pytest.fixture(scope="module")
def _contexts():
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx, arena_bytes=256 << 20, ws_bytes=1 << 20)
            ctx.guard = cm.__enter__()
            made[mode] = (ctx, cm)
        made[mode][0].guard.clear()
        return made[mode][0]

    yield get
    for ctx, cm in made.values():
        cm.__exit__(None, None, None)
        ctx.close()


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def _inputs(seed, p, d, zd):
    """Grid inputs whose pairs have ratios spread over a decade: row i + P repeats row i except on a share of the elements that grows
    with i.  P >= 3: pair 1 has identical latents, pair 2 identical images."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-256, 257, size=(2 * p, d)) / 256.0
    z = rs.randint(-256, 257, size=(2 * p, zd)) / 64.0
    for i in range(p):
        keep = rs.rand(d) > (i + 1.0) / p
        keep[rs.randint(d)] = False                      # (never the whole row)
        x[i + p, keep] = x[i, keep]
    if p >= 3:
        z[p + 1] = z[1]
        x[p + 2] = x[2]
    old = np.sign(rs.rand(2 * p, d) - 0.5) * (16.0 + rs.randint(0, 16, size=(2 * p, d)))        # what dx holds before accumulate = 1
    return x, z, old


def _label_variants(p):
    eq = np.full(2 * p, 4, np.int32)
    some = eq.copy()
    some[p] = 7                                          # pair 0 unequal
    if p >= 8:
        some[5] = 1                                      # ... and pair 5
    return {"none": None, "equal": eq, "some": some}


def _taus(ref_inf):
    """inf, and a clamp in the widest relative gap between the unmasked pairs' ratios (one pair: half its ratio -- clamped)."""
    r = np.sort(ref_inf["raw"][ref_inf["mask"] & (ref_inf["raw"] > 0)])
    if r.size == 0:
        return [np.inf, 0.25]
    if r.size == 1:
        return [np.inf, 0.5 * float(r[0])]
    k = int(np.argmax(r[1:] / r[:-1]))
    return [np.inf, float(np.sqrt(r[k] * r[k + 1]))]


def _call(ctx, p, d, zd, xd, zdv, lab, weight, tau, acc, old, want=(1, 1, 1)):
    from rcgan_amd import _lib as L
    loss = ctx.upload(np.array([L0], np.float32), L.F32)
    dx = ctx.upload(old) if acc else ctx.empty((2 * p, d))
    ratio = ctx.empty((p,), L.F32)
    rc = ctx.lib.rcgan_pair_diversity_fwd_bwd(ctx.h, p, d, zd, ctx.act_dtype, _p(xd), _p(zdv), _p(lab), weight, tau, _p(loss) if want[0] else None,
                                              _p(dx) if want[1] else None, acc, _p(ratio) if want[2] else None, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes)
    ctx.check(rc)
    return dict(loss=loss, dx=dx, ratio=ratio)


def _verify(ctx, mode, what, out, ref, p, d, acc, old, scale, tau):
    got_r, got_l, got_dx = (ctx.download(out[k]).astype(np.float64) for k in ("ratio", "loss", "dx"))
    mask = ref["mask"]
    print("%s: ratios %s loss %.9g (ref %.9g)" % (what, np.array2string(got_r, precision=6), got_l[0], L0 + ref["loss"]))
    assert np.array_equal(got_r[~mask], np.full(np.count_nonzero(~mask), -1.0)), what + ": the sentinel of masked pairs"
    assert (np.abs(got_r[mask] - ref["ratio"][mask]) <= 8 * _ulp32(ref["ratio"][mask])).all(), \
        "%s: ratio_out %r against %r" % (what, got_r, ref["ratio"])
    mag = abs(L0) + (WEIGHT / p) * np.abs(ref["terms"]).sum()
    assert abs(got_l[0] - (L0 + ref["loss"])) <= (p + 8) * _ulp32(mag), "%s: loss %.9g against %.9g" % (what, got_l[0], L0 + ref["loss"])
    want = ref["dx"]                                     # (scaled by the caller's `scale` already)
    if not acc:
        assert np.array_equal(np.sign(got_dx), np.sign(want)), what + ": sign / zero pattern of the gradient"
        err = np.abs(got_dx - want)
        bound = 8 * _ulp32(want) if mode == "f32" else np.abs(want) * (2.0 ** -8 if mode == "bf16" else 2.0 ** -10)
        assert (err <= bound).all(), "%s: gradient magnitude, worst error / bound %.3g" % (what, (err / np.maximum(bound, 1e-300)).max())
        assert np.isfinite(got_dx).all()
    else:
        push = np.concatenate([mask & ~ref["clamped"]] * 2)
        assert np.array_equal(got_dx[~push], old[~push]), what + ": a masked or clamped pair's accumulated rows changed"
        res = old + want
        ulp = _ulp32(res) if mode == "f32" else ULP16[mode] * 2.0 ** np.floor(np.log2(np.abs(res)))
        assert (np.abs(got_dx - res)[push] <= ulp[push]).all(), \
            "%s: accumulate, worst error %.3g ulp" % (what, (np.abs(got_dx - res)[push] / ulp[push]).max())


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_against_the_float64_reference(_contexts, mode):
    ctx = _contexts(mode)
    g = ctx.guard
    from rcgan_amd import _lib as L
    host_scale = 1024.0 if mode == "f16" else 1.0
    try:
        for gi, (p, d, zd) in enumerate((p, d, zd) for p in PAIRS for d in ROWS for zd in LATENTS):
            # one group of the fp16 cases reads half of its scale from device memory: 2048 * 0.5
            dev = ctx.upload(np.array([0.5], np.float32), L.F32) if (mode == "f16" and gi == 3) else None
            ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, host_scale * (2.0 if dev is not None else 1.0), _p(dev)))
            x, z, old = _inputs(100 + gi, p, d, zd)
            xd, zdv = ctx.upload(x), ctx.upload(z)
            assert np.array_equal(ctx.download(xd), x) and np.array_equal(ctx.download(zdv), z)      # the grids are exact in this dtype
            todo = []
            for lname, lab in _label_variants(p).items():
                labd = ctx.upload(lab) if lab is not None else None
                for tau in _taus(DR.pair_diversity(x, z, lab, WEIGHT, np.inf)):
                    ref = DR.pair_diversity(x, z, lab, WEIGHT, tau, scale=host_scale)
                    assert DR.min_relative_gap_to_tau(ref, tau) >= 1e-3
                    if np.isfinite(tau) and np.count_nonzero(ref["mask"] & (ref["raw"] > 0)) >= 2:
                        assert ref["clamped"].any() and (ref["mask"] & ~ref["clamped"]).any()        # the clamp splits the pairs
                    for acc in (0, 1):
                        what = "%s P %d D %d Z %d labels %s tau %g acc %d" % (mode, p, d, zd, lname, tau, acc)
                        todo.append((what, _call(ctx, p, d, zd, xd, zdv, labd, WEIGHT, tau, acc, old), ref, acc, tau))
            ctx.sync()
            g.check()
            for what, out, ref, acc, tau in todo:
                _verify(ctx, mode, what, out, ref, p, d, acc, old, host_scale, tau)
            if p >= 3:
                ref = todo[0][2]                         # labels none, tau inf: the identical-latents pair is masked, the identical-images pair
                assert not ref["mask"][1] and ref["mask"][2] and ref["ratio"][2] == 0.0              # counts with ratio 0 and no gradient
            g.clear()
    finally:
        ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1.0, None))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_optional_outputs_tight_workspace_repeat_and_replay(_contexts, mode):
    """Each optional output left out leaves the others' bits; the workspace of rcgan_pair_diversity_workspace_bytes(P) is enough and one
    float less is refused; a second call and a captured-and-replayed call give the first call's bits."""
    ctx = _contexts(mode)
    g = ctx.guard
    from rcgan_amd import _lib as L
    for d in (3072, 13):
        p, zd = 8, 128
        x, z, old = _inputs(7 + d, p, d, zd)
        lab = _label_variants(p)["some"]
        tau = _taus(DR.pair_diversity(x, z, lab, WEIGHT, np.inf))[1]
        xd, zdv, labd = ctx.upload(x), ctx.upload(z), ctx.upload(lab)
        need = ctx.lib.rcgan_pair_diversity_workspace_bytes(p)
        assert need == 4 * p
        with g.workspace(need):
            outs = [_call(ctx, p, d, zd, xd, zdv, labd, WEIGHT, tau, 1, old) for _ in range(2)]
            parts = [_call(ctx, p, d, zd, xd, zdv, labd, WEIGHT, tau, 1, old, want=w) for w in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
            ctx.sync()
            # captured: the buffers are made before the capture begins (an upload is not a launch of the library)
            loss = ctx.upload(np.array([L0], np.float32), L.F32)
            dx, ratio = ctx.upload(old), ctx.empty((p,), L.F32)
            ctx.sync()

            def body():
                ctx.check(ctx.lib.rcgan_pair_diversity_fwd_bwd(ctx.h, p, d, zd, ctx.act_dtype, _p(xd), _p(zdv), _p(labd), WEIGHT, tau, _p(loss), _p(dx), 1,
                                                               _p(ratio), C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            gid = ctx.capture(body)
            try:
                ctx.sync()
                assert g.unwritten(ratio) == p                              # capturing ran nothing
                ctx.graph_launch(gid)
                ctx.sync()
            finally:
                ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))
            cap = dict(loss=loss, dx=dx, ratio=ratio)
            g.check()
        with g.workspace(need - 4):
            small = ctx.empty((p,), L.F32)
            rc = ctx.lib.rcgan_pair_diversity_fwd_bwd(ctx.h, p, d, zd, ctx.act_dtype, _p(xd), _p(zdv), None, WEIGHT, tau, _p(outs[0]["loss"]), None, 0,
                                                      _p(small), C.c_void_p(ctx.ws_ptr), ctx.ws_bytes)
            assert rc == L.EWORKSPACE_TOO_SMALL
            ctx.sync()
            assert g.unwritten(small) == p
        first = {k: ctx.download(v) for k, v in outs[0].items()}
        for other in (outs[1], cap):
            for k, v in first.items():
                assert np.array_equal(ctx.download(other[k]).view(np.uint32), v.view(np.uint32)), (mode, d, k)
        for w, part in zip(("loss", "dx", "ratio"), parts):
            assert np.array_equal(ctx.download(part[w]).view(np.uint32), first[w].view(np.uint32)), (mode, d, w)
            for k in ("loss", "dx", "ratio"):
                if k != w and k != "dx":                                    # (dx was uploaded with the old values; the others are fresh)
                    if k == "loss":
                        assert ctx.download(part[k])[0] == np.float32(L0)
                    else:
                        assert g.unwritten(part[k]) == part[k].size
            if w != "dx":
                assert np.array_equal(ctx.download(part["dx"]), old.astype(np.float32))
        g.clear()


def test_invalid_arguments_launch_nothing(_contexts):
    ctx = _contexts("bf16")
    g = ctx.guard
    from rcgan_amd import _lib as L
    p, d, zd = 3, 24, 5
    x, z, _ = _inputs(1, p, d, zd)
    xd, zdv = ctx.upload(x), ctx.upload(z)
    lab = ctx.upload(np.zeros(2 * p, np.int32))
    loss, dx, ratio = ctx.empty((1,), L.F32), ctx.empty((2 * p, d)), ctx.empty((p,), L.F32)
    inf, nan = float("inf"), float("nan")
    ok = dict(p=p, d=d, zd=zd, dtype=ctx.act_dtype, x=xd.ptr, z=zdv.ptr, lab=lab.ptr, w=1.0, tau=0.5, loss=loss.ptr, dx=dx.ptr, ratio=ratio.ptr)
    bad = [dict(p=0), dict(p=-1), dict(d=0), dict(zd=0), dict(x=None), dict(z=None), dict(x=xd.ptr + 1), dict(z=zdv.ptr + 1), dict(dx=dx.ptr + 1),
           dict(lab=lab.ptr + 2), dict(loss=loss.ptr + 2), dict(ratio=ratio.ptr + 2), dict(w=nan), dict(w=inf), dict(w=-1.0), dict(w=-inf),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=nan), dict(tau=-inf), dict(dtype=99), dict(dtype=L.F16)]      # (F16: the OTHER 16-bit type here)

    def call(a, ws=None):
        v = lambda q: None if q is None else C.c_void_p(q)
        return ctx.lib.rcgan_pair_diversity_fwd_bwd(ctx.h, a["p"], a["d"], a["zd"], a["dtype"], v(a["x"]), v(a["z"]), v(a["lab"]), a["w"], a["tau"],
                                                    v(a["loss"]), v(a["dx"]), 0, v(a["ratio"]), C.c_void_p(ctx.ws_ptr if ws is None else ws), ctx.ws_bytes)
    for change in bad:
        assert call(dict(ok, **change)) == L.EINVALID_ARG, change
    assert call(ok, ws=ctx.ws_ptr + 2) == L.EINVALID_ARG
    # fp32 through the same library: 2-byte alignment is not enough
    assert call(dict(ok, dtype=L.F32, x=xd.ptr + 2)) == L.EINVALID_ARG
    # weight 0 is valid, launches nothing and touches nothing
    assert call(dict(ok, w=0.0)) == 0
    ctx.sync()
    g.check()
    for t in (loss, dx, ratio):
        assert g.unwritten(t) == t.size
    # ... and the same arguments with a weight run
    assert call(ok) == 0
    ctx.sync()
    g.check()
    assert g.unwritten(dx) == 0 and g.unwritten(ratio) == 0


def test_tape_op_adds_to_an_existing_gradient_and_takes_none_for_z(_contexts):
    """ops.pair_diversity: a tensor without a gradient gets one (accumulate = 0); one that has a gradient gets the term added; z gets
    none; outside a recording nothing is written but the loss and the ratios."""
    ctx = _contexts("f32")
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    p, d, zd = 3, 24, 5
    x, z, old = _inputs(2, p, d, zd)
    ref = DR.pair_diversity(x, z, None, WEIGHT, np.inf)
    res = []
    for pre in (False, True):
        xd, zdv = ctx.upload(x), ctx.upload(z)
        xd.req, zdv.req = True, True
        if pre:
            xd.grad = ctx.upload(old)
        loss, ratio = ctx.upload(np.array([0.0], np.float32), L.F32), ctx.empty((p,), L.F32)
        O.pair_diversity(ctx, xd, zdv, None, WEIGHT, np.inf, loss, ratio_out=ratio)
        assert zdv.grad is None
        res.append((ctx.download(xd.grad), ctx.download(loss)[0]))
    np.testing.assert_allclose(res[0][0], ref["dx"], rtol=1e-6)
    np.testing.assert_allclose(res[1][0], old + ref["dx"], rtol=1e-6)
    assert res[0][1] == res[1][1] and abs(res[0][1] - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    ctx.recording = False
    try:
        xd = ctx.upload(x)
        xd.req = True
        loss = ctx.upload(np.array([0.0], np.float32), L.F32)
        O.pair_diversity(ctx, xd, ctx.upload(z), None, WEIGHT, np.inf, loss)
        assert xd.grad is None and ctx.download(loss)[0] == res[0][1]
    finally:
        ctx.recording = True
    with pytest.raises(ValueError, match="pair_diversity"):
        O.pair_diversity(ctx, ctx.upload(x[:5]), ctx.upload(z[:5]), None, WEIGHT, np.inf, loss)
