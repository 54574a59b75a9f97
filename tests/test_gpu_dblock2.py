"""The 16x16 down block of the CIFAR critic (D.Block.2) with its forward as ONE launch (csrc/conv_dblock2.hip, ops.d_block2) against the
same block built from the four forward calls it replaces (meanpool2, the 1x1 shortcut, the register-filter Conv1, Conv2 + pool as one 4x4
stride-2 convolution).  The rounding points are the same on both sides, so h (Conv1's output) and xp (the pooled input) must be bit-equal
and y may differ by the fp32 summation order inside Conv2 only: TOL[mode], the bound test_d_trunk_equals_layerwise_blocks uses for the
same reason; and 3 TOL[mode] against a float64 restatement with the 16-bit rounding between layers.  At the production batch, where the
four launches are the kernels whose summation order the fused kernel follows, y must be bit-equal too.  Every run is inside guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nn
from tests.guard import guarded
from tests.gpu_util import FakeParam, assert_close, half_round, make_ctx, rel_err

pytestmark = pytest.mark.gpu

TOL = {"bf16": 1e-2, "f16": 3e-3}         # tests/test_gpu_ops.py
SIGMA = 1.3


@pytest.fixture(scope="module", params=["bf16", "f16"])
def dev(request):
    ctx = make_ctx(request.param, arena=1 << 20)          # (its own arena is replaced by the guarded one)
    cm = guarded(ctx)
    ctx.guard = cm.__enter__()
    yield ctx, request.param
    cm.__exit__(None, None, None)
    ctx.close()


def _weights(seed):
    rs = np.random.RandomState(1000 + seed)
    w = dict(ws=(rs.randn(1, 1, 128, 128) / np.sqrt(128) * 1.2), w1=(rs.randn(3, 3, 128, 128) / np.sqrt(9 * 128) * 1.2),
             w2=(rs.randn(3, 3, 128, 128) / np.sqrt(9 * 128) * 1.2))
    b = dict(bs=0.1 * rs.randn(128), b1=0.1 * rs.randn(128), b2=0.1 * rs.randn(128))
    return {k: v.astype(np.float32) for k, v in {**w, **b}.items()}


def _block(ctx, x, P, fused, dy=None):
    """One forward (and, with dy, the backward pass) of the block on fresh parameters; fused: ops.d_block2, else the four calls."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx.new_step()
    ctx.guard.clear()
    xd = ctx.upload(x)
    xd.req = dy is not None
    fp = {k: FakeParam(ctx, v) for k, v in P.items()}
    W = {k: O.Weight(ctx, fp[k].t, ctx.upload(np.array([SIGMA], np.float32), L.F32)) for k in ("ws", "w1", "w2")}
    d = L.ConvDesc(1, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    if fused:
        _, frag = O.fragments_batch(ctx, None, [(W["w1"], d)], dblock2=(W["w2"], W["ws"]))
        assert O.d_block2_ok(ctx, xd, W["w1"], frag)
        saved = []
        y = O.d_block2(ctx, xd, W["ws"], fp["bs"].t, W["w1"], fp["b1"].t, W["w2"], fp["b2"].t, frag=frag, _saved=saved)
        h, xp = saved
    else:
        O.fragments_batch(ctx, None, [(W["w1"], d)])
        xp = O.meanpool2(ctx, xd)
        t = O.conv2d(ctx, xp, W["ws"], fp["bs"].t, 1)
        h = O.conv2d(ctx, xd, W["w1"], fp["b1"].t, 3, in_relu=True)
        y = O.conv2d_meanpool(ctx, h, W["w2"], fp["b2"].t, in_relu=True, accumulate_into=t)
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(h) == 0 and ctx.guard.unwritten(xp) == 0 and ctx.guard.unwritten(y) == 0
    raw = lambda t: ctx.view(t).view(torch.int16).cpu().numpy().copy()
    out = dict(y=ctx.download(y), h_bits=raw(h), xp_bits=raw(xp), y_bits=raw(y))
    if dy is not None:
        y.grad = ctx.upload(dy)
        ctx.backward()
        ctx.sync()
        ctx.guard.check()
        out.update(dx=ctx.download(xd.grad), dw={k: ctx.download(W[k].dwbar) for k in W}, db={k: fp[k].grad(ctx) for k in ("bs", "b1", "b2")})
    return out


def _oracle(mode, x, P):
    """float64 with the 16-bit rounding between layers restated (as test_d_trunk_equals_layerwise_blocks restates the 8x8 stage)."""
    q = lambda v: half_round(mode, v).astype(np.float64)
    x = x.astype(np.float64)
    wq = {k: q(P[k] / np.float32(SIGMA)) for k in ("ws", "w1", "w2")}
    h = q(nn.conv2d_fwd(np.maximum(x, 0), wq["w1"]) + P["b1"])
    t = q(nn.conv2d_fwd(q(nn.meanpool2(x)), wq["ws"]) + P["bs"])
    return q(t + nn.meanpool2(nn.conv2d_fwd(np.maximum(h, 0), wq["w2"])) + P["b2"])


def _compare(ctx, mode, x, seed, oracle=True):
    P = _weights(seed)
    a, b = _block(ctx, x, P, True), _block(ctx, x, P, False)
    assert np.array_equal(a["xp_bits"], b["xp_bits"]), "xp differs in %d elements" % int((a["xp_bits"] != b["xp_bits"]).sum())
    assert np.array_equal(a["h_bits"], b["h_bits"]), "h differs in %d elements" % int((a["h_bits"] != b["h_bits"]).sum())
    assert_close(a["y"], b["y"], TOL[mode], "fused y vs four launches")
    if oracle:
        assert_close(a["y"], _oracle(mode, x, P), 3 * TOL[mode], "fused y vs float64 restatement")


@pytest.mark.parametrize("n", [1, 3])
def test_fused_equals_four_launches(dev, n):
    """n = 1: two workgroups; n = 3: an odd grid.  Guard bands of every buffer untouched, no output element left unwritten (_block)."""
    ctx, mode = dev
    x = half_round(mode, np.random.RandomState(n).randn(n, 16, 16, 128))
    _compare(ctx, mode, x, n)


@pytest.mark.parametrize("kind", ["middle_rows", "frame"])
def test_halo_row_and_image_edges(dev, kind):
    """Inputs whose only support is rows 6..9 (everything the two halves must agree on: rows 7 and 8 of h are computed by both) or the
    image's frame (rows 0 and 15, columns 0 and 15: the clipped patch rows, the zero halo, the zero row of relu(h))."""
    ctx, mode = dev
    full = np.random.RandomState(7).randn(2, 16, 16, 128)
    x = np.zeros_like(full)
    if kind == "middle_rows":
        x[:, 6:10] = full[:, 6:10]
    else:
        x[:, [0, 15]] = full[:, [0, 15]]
        x[:, :, [0, 15]] = full[:, :, [0, 15]]
    _compare(ctx, mode, half_round(mode, x), 11)


def test_production_batch_forward_and_unchanged_backward(dev):
    """n = 128 (256 workgroups, one per CU): forward as above; then ctx.backward() through the four unchanged backward entries, compared in
    the norm with the bound the 8x8 stage's test uses at this size -- pre-activations within summation noise of zero flip their ReLU mask
    (only Conv2's output differs between the routes, so here only through y's consumers; the bound is kept the same)."""
    ctx, mode = dev
    n = 128
    rs = np.random.RandomState(128)
    x = half_round(mode, rs.randn(n, 16, 16, 128))
    dy = half_round(mode, rs.randn(n, 8, 8, 128))
    P = _weights(128)
    a, b = _block(ctx, x, P, True, dy), _block(ctx, x, P, False, dy)
    assert np.array_equal(a["xp_bits"], b["xp_bits"]) and np.array_equal(a["h_bits"], b["h_bits"])
    assert_close(a["y"], b["y"], TOL[mode], "fused y vs four launches")
    # At this size the four launches are the kernels of the training step (the shortcut on the 64 x 64 tile kernel, Conv2 on its gather
    # form with the reduction dealt to two wavefront groups), and the fused kernel sums in their order: the block output has their bits,
    # so a training run through the fused forward computes what it computed through the four launches.
    differ = int((a["y_bits"] != b["y_bits"]).sum())
    print("n = 128 %s: %d of %d elements of y differ in their bits" % (mode, differ, a["y_bits"].size))
    assert differ == 0, "y differs from the four launches in %d elements" % differ
    tol = 2e-2
    assert rel_err(a["dx"], b["dx"]) < tol, rel_err(a["dx"], b["dx"])
    for k in ("ws", "w1", "w2"):
        assert rel_err(a["dw"][k], b["dw"][k]) < tol, (k, rel_err(a["dw"][k], b["dw"][k]))
    for k in ("bs", "b1", "b2"):
        assert rel_err(a["db"][k], b["db"][k]) < tol, (k, rel_err(a["db"][k], b["db"][k]))


def test_refusals(dev):
    """rcgan_dblock2_ok takes D.Block.2's Conv1 descriptor and nothing else; the entry point refuses what it refuses and launches nothing."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    lib, dt = ctx.lib, ctx.act_dtype
    other = L.F16 if dt == L.BF16 else L.BF16
    some = C.c_void_p(ctx.empty((64,), L.F32).ptr)
    ok = lambda d, a=some, b=some: lib.rcgan_dblock2_ok(C.byref(d) if d is not None else None, a, b)
    good = lambda n: L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU)
    for n in (1, 3, 128, 4000):
        assert ok(good(n)) == 1
    bad = [L.ConvDesc(4, 8, 8, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 32, 32, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 8, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 8, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 16, 64, 128, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 16, 16, 128, 64, 3, 3, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 16, 256, 256, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 16, 16, 128, 256, 3, 3, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 16, 128, 128, 1, 1, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 16, 16, 128, 128, 5, 5, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 2, dt, L.CONV_IN_RELU), L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 1, L.F32, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 1, other, L.CONV_IN_RELU), L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 1, dt, 0),
           L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU | L.CONV_ACCUMULATE),
           L.ConvDesc(4, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU | L.CONV_OUT_MEANPOOL2),
           L.ConvDesc(0, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(1 << 16, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU)]
    for d in bad:
        assert ok(d) == 0, tuple(getattr(d, f) for f, _ in d._fields_)
    assert ok(None) == 0 and ok(good(4), None, some) == 0 and ok(good(4), some, None) == 0
    ctx.new_step()
    ctx.guard.clear()
    out = ctx.empty((64,), ctx.act_dtype)
    p = C.c_void_p(out.ptr)
    for d in bad[:3]:
        assert lib.rcgan_dblock2_fwd(ctx.h, C.byref(d), p, p, p, p, p, p, p, p, p) != 0
        assert b"rcgan_dblock2_ok" in lib.rcgan_last_error(ctx.h)
    assert lib.rcgan_dblock2_fwd(ctx.h, C.byref(good(1)), None, p, p, p, p, p, p, p, p) == L.EINVALID_ARG
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(out) == out.size


def test_discriminator_takes_the_fused_block_or_the_four_launches(monkeypatch):
    """The CIFAR critic step calls ops.d_block2 by default; with the switch off rcgan_dblock2_ok has no copies to say yes to and the same
    step runs the four launches (ops.d_block2 is never entered)."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import ops as O
    from rcgan_amd.cifar import CifarRCGAN, create_variables
    B = 4
    rs = np.random.RandomState(0)
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", use_graphs=False, device_rng=False,
                   variables=create_variables(0, "rcgan"), arena_bytes=1 << 30)
    try:
        lab = rs.randint(10, size=B)
        m.set_inputs(images=rs.randint(0, 256, size=(B, 3072)), noise=rs.uniform(0, 1 / 128., size=(B, 3072)).astype(np.float32),
                     labels=lab, labels_random=rs.randint(10, size=B), labels_biased=rs.randint(10, size=B),
                     inv_weights=np.eye(10, dtype=np.float32)[lab], z=rs.randn(B, 128).astype(np.float32),
                     labels_all=np.concatenate([lab, lab]))
        calls, real = [], O.d_block2
        monkeypatch.setattr(O, "d_block2", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        cost_fused = m.eval_d_cost()
        assert len(calls) >= 1
        monkeypatch.setattr(O, "FUSED_DBLOCK2", False)
        seen = len(calls)
        cost_four = m.eval_d_cost()
        assert len(calls) == seen
        # (each evaluation moves the spectral norms' u vectors on, so the two costs are not the same number: the values are compared
        # at op level above and by the step tests, which now run through the fused forward)
        assert np.isfinite(cost_fused) and np.isfinite(cost_four), (cost_fused, cost_four)
    finally:
        m.ctx.close()


def test_graph_replay_gives_the_eager_bytes(dev):
    """The launch captured into a graph and replayed twice writes the bytes of the eager call (all buffers allocated before the capture)."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx, mode = dev
    n = 3
    x = half_round(mode, np.random.RandomState(21).randn(n, 16, 16, 128))
    P = _weights(21)
    ctx.new_step()
    ctx.guard.clear()
    xd = ctx.upload(x)
    fp = {k: FakeParam(ctx, v) for k, v in P.items()}
    W = {k: O.Weight(ctx, fp[k].t, ctx.upload(np.array([SIGMA], np.float32), L.F32)) for k in ("ws", "w1", "w2")}
    d1 = L.ConvDesc(1, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    _, frag = O.fragments_batch(ctx, None, [(W["w1"], d1)], dblock2=(W["w2"], W["ws"]))
    d = L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    outs = [[ctx.empty(s, ctx.act_dtype) for s in ((n, 16, 16, 128), (n, 8, 8, 128), (n, 8, 8, 128))] for _ in range(2)]
    p = lambda t: C.c_void_p(t.ptr)
    call = lambda o: ctx.check(ctx.lib.rcgan_dblock2_fwd(ctx.h, C.byref(d), p(xd), p(W["w1"].rf_frag), p(frag), p(fp["b1"].t), p(fp["b2"].t),
                                                         p(fp["bs"].t), p(o[0]), p(o[1]), p(o[2])))
    call(outs[0])
    ctx.sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=ctx.stream):
        call(outs[1])
    ctx.sync()
    assert all(ctx.guard.unwritten(t) == t.size for t in outs[1])           # capturing ran nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    ctx.guard.check()
    for a, b in zip(*outs):
        assert ctx.view(a).view(torch.int16).cpu().numpy().tobytes() == ctx.view(b).view(torch.int16).cpu().numpy().tobytes()
    del graph
