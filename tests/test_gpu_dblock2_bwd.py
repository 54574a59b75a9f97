"""The 16x16 down block of the CIFAR critic (D.Block.2) with its data gradient as ONE launch (csrc/conv_dblock2_bwd.hip, the backward entry
of ops.d_block2 under FUSED_DBLOCK2_BWD) against the four backward entries it replaces (Conv2 + pool's data gradient in its sub-pixel form,
the register-filter Conv1 data gradient, the 1x1 shortcut's, the pool's adjoint accumulated into dx).  Both sides run the SAME fused
forward, so h and the masks are the same bits; only the backward switch differs.  The rounding points are the same on both sides (dh, dxp,
the intermediate dx, dx), so the results may differ by the fp32 summation order of the sub-pixel stage only (small batches take the tile
kernel with two K-split groups): TOL[mode], and 3 TOL[mode] against a float64 restatement with the 16-bit rounding points -- the bounds of
tests/test_gpu_dblock2.py.  At the production batch the four launches are the kernels whose summation order the fused kernel follows: dh
and dx must be bit-equal, and with them every filter and bias gradient of the grouped launch.  Every run is inside guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nn
from tests.guard import guarded
from tests.gpu_util import FakeParam, assert_close, half_round, make_ctx, rel_err

pytestmark = pytest.mark.gpu

TOL = {"bf16": 1e-2, "f16": 3e-3}         # tests/test_gpu_dblock2.py
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


def _block(ctx, monkeypatch, x, P, dy, fused_bwd, second_consumer=None):
    """The fused forward and the backward pass of the block on fresh parameters; fused_bwd: the value of ops.FUSED_DBLOCK2_BWD.
    second_consumer: the gradient of a 2x2 mean of x recorded behind the block, so x has a gradient when the block's entry runs."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    monkeypatch.setattr(O, "FUSED_DBLOCK2_BWD", fused_bwd)
    calls, real = [], O.d_block2_bwd
    monkeypatch.setattr(O, "d_block2_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ctx.new_step()
    ctx.guard.clear()
    xd = ctx.upload(x)
    xd.req = True
    fp = {k: FakeParam(ctx, v) for k, v in P.items()}
    W = {k: O.Weight(ctx, fp[k].t, ctx.upload(np.array([SIGMA], np.float32), L.F32)) for k in ("ws", "w1", "w2")}
    d = L.ConvDesc(1, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    _, frag = O.fragments_batch(ctx, None, [(W["w1"], d)], dblock2=(W["w2"], W["ws"]))
    assert O.d_block2_ok(ctx, xd, W["w1"], frag)
    saved = []
    y = O.d_block2(ctx, xd, W["ws"], fp["bs"].t, W["w1"], fp["b1"].t, W["w2"], fp["b2"].t, frag=frag, _saved=saved)
    h, xp = saved
    if second_consumer is not None:
        z = O.meanpool2(ctx, xd)
        z.grad = ctx.upload(second_consumer)
    y.grad = ctx.upload(dy)
    ctx.backward()
    ctx.sync()
    ctx.guard.check()
    dh, dx = h.grad, xd.grad
    assert ctx.guard.unwritten(dh) == 0 and ctx.guard.unwritten(dx) == 0
    raw = lambda t: ctx.view(t).view(torch.int16).cpu().numpy().copy()
    return dict(h=ctx.download(h), dh=ctx.download(dh), dx=ctx.download(dx), dh_bits=raw(dh), dx_bits=raw(dx),
                dxp=ctx.download(xp.grad) if xp.grad is not None else None, calls=len(calls),
                dw={k: ctx.download(W[k].dwbar) for k in W}, db={k: fp[k].grad(ctx) for k in ("bs", "b1", "b2")})


def _oracle(mode, x, h, dy, P):
    """float64 with the 16-bit rounding points restated: dh, dxp, the intermediate dx, dx.  h: the forward's (the mask both sides use)."""
    q = lambda v: half_round(mode, v).astype(np.float64)
    dy = dy.astype(np.float64)
    wq = {k: q(P[k] / np.float32(SIGMA)) for k in ("ws", "w1", "w2")}
    dh = q((h > 0) * nn.conv2d_bwd_input(nn.meanpool2_bwd(dy), wq["w2"], h.shape))
    dxp = q(nn.conv2d_bwd_input(dy, wq["ws"], dy.shape))
    dxc = q((x > 0) * nn.conv2d_bwd_input(dh, wq["w1"], x.shape))
    return dh, q(dxc + nn.meanpool2_bwd(dxp))


def _compare(ctx, monkeypatch, mode, x, dy, seed, P=None):
    P = _weights(seed) if P is None else P
    a, b = _block(ctx, monkeypatch, x, P, dy, True), _block(ctx, monkeypatch, x, P, dy, False)
    assert a["calls"] == 1 and b["calls"] == 0
    assert np.array_equal(a["h"], b["h"])
    assert_close(a["dh"], b["dh"], TOL[mode], "fused dh vs four launches")
    assert_close(a["dx"], b["dx"], TOL[mode], "fused dx vs four launches")
    dh, dx = _oracle(mode, x, a["h"], dy, P)
    assert_close(a["dh"], dh, 3 * TOL[mode], "fused dh vs float64 restatement")
    assert_close(a["dx"], dx, 3 * TOL[mode], "fused dx vs float64 restatement")
    return a, b


@pytest.mark.parametrize("n", [1, 3])
def test_fused_equals_four_launches(dev, monkeypatch, n):
    """n = 1: two workgroups; n = 3: an odd grid.  Guard bands of every buffer untouched, no element of dh or dx left unwritten (_block)."""
    ctx, mode = dev
    rs = np.random.RandomState(40 + n)
    x = half_round(mode, rs.randn(n, 16, 16, 128))
    dy = half_round(mode, rs.randn(n, 8, 8, 128))
    _compare(ctx, monkeypatch, mode, x, dy, n)


@pytest.mark.parametrize("kind", ["middle_rows", "frame"])
def test_halo_row_and_image_edges(dev, monkeypatch, kind):
    """dy supported only on pooled rows 3 and 4 (the rows both halves read: rows 7 and 8 of dh are computed by both) or on the frame
    (pooled rows and columns 0 and 7: the clipped patch rows, the zero halo of dy, the zero row of the dh patch)."""
    ctx, mode = dev
    rs = np.random.RandomState(47)
    x = half_round(mode, rs.randn(2, 16, 16, 128))
    full = rs.randn(2, 8, 8, 128)
    dy = np.zeros_like(full)
    if kind == "middle_rows":
        dy[:, 3:5] = full[:, 3:5]
    else:
        dy[:, [0, 7]] = full[:, [0, 7]]
        dy[:, :, [0, 7]] = full[:, :, [0, 7]]
    _compare(ctx, monkeypatch, mode, x, half_round(mode, dy), 51)


@pytest.mark.parametrize("kind", ["h_nonpositive", "x_nonpositive"])
def test_masks(dev, monkeypatch, kind):
    """b1 = -100: h <= 0 everywhere, so dh is all zero bits; x <= 0 everywhere: Conv1's part of dx vanishes.  Either way dx is exactly
    16bit(0.25 spread(dxp)) of the four launches' dxp (the 1x1 data gradient takes the same kernel at every batch)."""
    ctx, mode = dev
    rs = np.random.RandomState(53)
    x = half_round(mode, rs.randn(2, 16, 16, 128))
    dy = half_round(mode, rs.randn(2, 8, 8, 128))
    P = _weights(53)
    if kind == "h_nonpositive":
        P["b1"] = np.full(128, -100.0, np.float32)
    else:
        x = -np.abs(x)
    a, b = _compare(ctx, monkeypatch, mode, x, dy, 53, P)
    if kind == "h_nonpositive":
        assert (a["h"] <= 0).all()
        assert not a["dh_bits"].any(), "dh has %d non-zero bit patterns" % int((a["dh_bits"] != 0).sum())
    want = half_round(mode, nn.meanpool2_bwd(b["dxp"].astype(np.float32)))
    assert np.array_equal(a["dx"], want), "dx differs from 16bit(0.25 spread(dxp)) in %d elements" % int((a["dx"] != want).sum())
    assert np.array_equal(a["dx_bits"], b["dx_bits"])


def test_production_batch_bit_equal(dev, monkeypatch):
    """n = 128 (256 workgroups, one per CU): the four launches are the kernels of the training step (the sub-pixel form and the 1x1 on
    the 64 x 64 tile kernel with one K chain, Conv1 on the register-filter kernel) and the fused kernel sums in their order: dh and dx have
    their bits, hence the grouped filter-gradient launch reads the same operands and every dw and db is equal."""
    ctx, mode = dev
    n = 128
    rs = np.random.RandomState(128)
    x = half_round(mode, rs.randn(n, 16, 16, 128))
    dy = half_round(mode, rs.randn(n, 8, 8, 128))
    P = _weights(128)
    a, b = _block(ctx, monkeypatch, x, P, dy, True), _block(ctx, monkeypatch, x, P, dy, False)
    assert a["calls"] == 1 and b["calls"] == 0
    for k in ("dh", "dx"):
        differ = int((a[k + "_bits"] != b[k + "_bits"]).sum())
        print("n = 128 %s: %d of %d elements of %s differ in their bits" % (mode, differ, a[k + "_bits"].size, k))
        assert differ == 0, "%s differs from the four launches in %d elements" % (k, differ)
    for k in ("ws", "w1", "w2"):
        assert np.array_equal(a["dw"][k], b["dw"][k]), k
    for k in ("bs", "b1", "b2"):
        assert np.array_equal(a["db"][k], b["db"][k]), k


def test_fallback_when_x_has_a_gradient(dev, monkeypatch):
    """A second consumer of x whose entry runs first: the block's entry finds x.grad and runs the four entries -- the result of the
    switch being off, bit for bit, and the fused entry point is not called."""
    ctx, mode = dev
    rs = np.random.RandomState(59)
    x = half_round(mode, rs.randn(2, 16, 16, 128))
    dy = half_round(mode, rs.randn(2, 8, 8, 128))
    dz = half_round(mode, rs.randn(2, 8, 8, 128))
    P = _weights(59)
    a, b = _block(ctx, monkeypatch, x, P, dy, True, dz), _block(ctx, monkeypatch, x, P, dy, False, dz)
    assert a["calls"] == 0 and b["calls"] == 0
    assert np.array_equal(a["dh_bits"], b["dh_bits"]) and np.array_equal(a["dx_bits"], b["dx_bits"])
    for k in ("ws", "w1", "w2"):
        assert np.array_equal(a["dw"][k], b["dw"][k]), k


def _launch_setup(ctx, mode, n, seed):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    rs = np.random.RandomState(seed)
    P = _weights(seed)
    ctx.new_step()
    ctx.guard.clear()
    up = lambda shape: ctx.upload(half_round(mode, rs.randn(*shape)))
    dy, h, x = up((n, 8, 8, 128)), up((n, 16, 16, 128)), up((n, 16, 16, 128))
    fp = {k: FakeParam(ctx, v) for k, v in P.items()}
    W = {k: O.Weight(ctx, fp[k].t, ctx.upload(np.array([SIGMA], np.float32), L.F32)) for k in ("ws", "w1", "w2")}
    d1 = L.ConvDesc(1, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    _, frag = O.fragments_batch(ctx, None, [(W["w1"], d1)], dblock2=(W["w2"], W["ws"]))
    return dy, h, x, W["w1"].rf_frag, frag


def test_graph_replay_gives_the_eager_bytes(dev):
    """The launch captured into a graph and replayed twice writes the bytes of the eager call (all buffers allocated before the capture)."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    n = 3
    dy, h, x, frag1, frag = _launch_setup(ctx, mode, n, 61)
    d = L.ConvDesc(n, 16, 16, 128, 128, 3, 3, 1, ctx.act_dtype, L.CONV_IN_RELU)
    outs = [[ctx.empty((n, 16, 16, 128), ctx.act_dtype) for _ in range(2)] for _ in range(2)]
    p = lambda t: C.c_void_p(t.ptr)
    call = lambda o: ctx.check(ctx.lib.rcgan_dblock2_bwd(ctx.h, C.byref(d), p(dy), p(h), p(x), p(frag1), p(frag), p(o[0]), p(o[1])))
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
        assert ctx.guard.unwritten(a) == 0
        assert ctx.view(a).view(torch.int16).cpu().numpy().tobytes() == ctx.view(b).view(torch.int16).cpu().numpy().tobytes()
    del graph


def test_refusals(dev):
    """rcgan_dblock2_bwd refuses what rcgan_dblock2_ok refuses and a null operand, and launches nothing."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    lib, dt = ctx.lib, ctx.act_dtype
    ctx.new_step()
    ctx.guard.clear()
    out = ctx.empty((64,), ctx.act_dtype)
    p = C.c_void_p(out.ptr)
    bad = [L.ConvDesc(4, 8, 8, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU), L.ConvDesc(4, 32, 32, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU),
           L.ConvDesc(4, 16, 8, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU)]
    for d in bad:
        assert lib.rcgan_dblock2_ok(C.byref(d), p, p) == 0
        assert lib.rcgan_dblock2_bwd(ctx.h, C.byref(d), p, p, p, p, p, p, p) != 0
        assert b"rcgan_dblock2_ok" in lib.rcgan_last_error(ctx.h)
    good = L.ConvDesc(1, 16, 16, 128, 128, 3, 3, 1, dt, L.CONV_IN_RELU)
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert lib.rcgan_dblock2_bwd(ctx.h, C.byref(good), *args) == L.EINVALID_ARG, hole
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(out) == out.size


def test_critic_step_with_and_without_the_fused_backward(monkeypatch):
    """One d_step of the CIFAR critic from the same variables with the backward switch on and off: every parameter and every critic
    gradient agrees within the step-level bound of tests/test_gpu_dblock2.py, and the fused entry ran in the first step only."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import ops as O
    from rcgan_amd.cifar import CifarRCGAN, create_variables
    B = 4
    calls, real = [], O.d_block2_bwd
    monkeypatch.setattr(O, "d_block2_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = []
    for on in (True, False):
        monkeypatch.setattr(O, "FUSED_DBLOCK2_BWD", on)
        rs = np.random.RandomState(0)
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", use_graphs=False, device_rng=False,
                       variables=create_variables(0, "rcgan"), arena_bytes=1 << 30)
        try:
            lab = rs.randint(10, size=B)
            m.set_inputs(images=rs.randint(0, 256, size=(B, 3072)), noise=rs.uniform(0, 1 / 128., size=(B, 3072)).astype(np.float32),
                         labels=lab, labels_random=rs.randint(10, size=B), labels_biased=rs.randint(10, size=B),
                         inv_weights=np.eye(10, dtype=np.float32)[lab], z=rs.randn(B, 128).astype(np.float32),
                         labels_all=np.concatenate([lab, lab]))
            seen = len(calls)
            m.d_step(iteration=0)
            assert (len(calls) > seen) == on
            got.append((m.get_params(), m.get_grads(m.PD)))
        finally:
            m.ctx.close()
    tol = 2e-2
    for which in (0, 1):
        for k, v in got[0][which].items():
            assert np.isfinite(v).all(), k
            assert rel_err(v, got[1][which][k]) < tol, (which, k, rel_err(v, got[1][which][k]))
