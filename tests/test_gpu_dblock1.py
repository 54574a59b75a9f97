"""The 32x32 input block of the CIFAR critic (D.Block.1) with its forward as ONE launch (csrc/conv_dblock1.hip, ops.d_block1) against the
same block built from the forward calls it replaces (meanpool2, the 1x1 shortcut and the 3x3 Conv1 on the image-end kernel, Conv2 + pool
as one 4x4 stride-2 convolution).  The rounding points are the same on both sides, so h (Conv1's output), xp (the pooled input) and t (the
shortcut) must be bit-equal and y may differ by the fp32 summation order inside Conv2 only: TOL[mode]; and 3 TOL[mode] against a float64
restatement with the 16-bit rounding at the four points.  At the production batch, where the three launches are the kernels whose
summation order the fused kernel follows, y must be bit-equal too.  Every run is inside guard bands."""
import numpy as np
import pytest
import torch

from oracle import nn
from tests.guard import guarded
from tests.gpu_util import FakeParam, assert_close, half_round, make_ctx

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
    rs = np.random.RandomState(2000 + seed)
    w = dict(ws=(rs.randn(1, 1, 3, 128) / np.sqrt(3) * 1.2), w1=(rs.randn(3, 3, 3, 128) / np.sqrt(27) * 1.2),
             w2=(rs.randn(3, 3, 128, 128) / np.sqrt(9 * 128) * 1.2))
    b = dict(bs=0.1 * rs.randn(128), b1=0.1 * rs.randn(128), b2=0.1 * rs.randn(128))
    return {k: v.astype(np.float32) for k, v in {**w, **b}.items()}


def _block(ctx, x, P, fused, dy=None, given_pool=False, y_host=True):
    """One forward (and, with dy, the backward pass) of the block on fresh parameters; fused: ops.d_block1, else the three calls (and the
    pool).  given_pool: the pooled images exist already, as in the critic step (Graph.image_pool): the fused launch must not store them."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx.new_step()
    ctx.guard.clear()
    xd = ctx.upload(x)
    xd.req = dy is not None
    fp = {k: FakeParam(ctx, v) for k, v in P.items()}
    W = {k: O.Weight(ctx, fp[k].t, ctx.upload(np.array([SIGMA], np.float32), L.F32)) for k in ("ws", "w1", "w2")}
    pooled = O.meanpool2(ctx, ctx.upload(x)) if given_pool else None
    raw = lambda t: ctx.view(t).view(torch.int16).clone()
    pooled_before = raw(pooled) if given_pool else None
    before = len(ctx.guard.arena.bodies)
    if fused:
        _, _, frag = O.fragments_batch(ctx, None, [], dblock1=W["w2"])
        assert O.d_block1_ok(ctx, xd, frag)
        saved = []
        y = O.d_block1(ctx, xd, W["ws"], fp["bs"].t, W["w1"], fp["b1"].t, W["w2"], fp["b2"].t, frag=frag, pooled=pooled, _saved=saved)
        h, xp = saved
    else:
        xp = pooled if given_pool else O.meanpool2(ctx, xd)
        t = O.conv2d(ctx, xp, W["ws"], fp["bs"].t, 1)
        h = O.conv2d(ctx, xd, W["w1"], fp["b1"].t, 3)
        y = O.conv2d_meanpool(ctx, h, W["w2"], fp["b2"].t, in_relu=True, accumulate_into=t)
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(h) == 0 and ctx.guard.unwritten(xp) == 0 and ctx.guard.unwritten(y) == 0
    if given_pool:
        # nothing was stored over, beside or instead of the given pooled images: same bits, same tensor, no buffer of the pool's size
        assert xp is pooled and torch.equal(raw(pooled), pooled_before)
        if fused:
            sizes = [b - a for a, b in ctx.guard.arena.bodies[before:]]
            assert pooled.nbytes not in sizes, sizes
    out = dict(h_bits=raw(h), xp_bits=raw(xp), y_bits=raw(y))
    if y_host:
        out["y"] = ctx.download(y)
    if dy is not None:
        y.grad = ctx.upload(dy)
        ctx.backward()
        ctx.sync()
        ctx.guard.check()
        out.update(dx=ctx.download(xd.grad), dw={k: ctx.download(W[k].dwbar) for k in W}, db={k: fp[k].grad(ctx) for k in ("bs", "b1", "b2")})
    return out


def _shortcut_bits(ctx, x, P):
    """t on both sides.  Fused: with Conv2's filter and bias zero the launch's y is 16bit((0 + 0) + t) = t.  Unfused: the shortcut alone."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    Z = dict(P, w2=np.zeros_like(P["w2"]), b2=np.zeros_like(P["b2"]))
    fused = _block(ctx, x, Z, True, y_host=False)["y_bits"]
    ctx.new_step()
    ctx.guard.clear()
    ws = O.Weight(ctx, FakeParam(ctx, P["ws"]).t, ctx.upload(np.array([SIGMA], np.float32), L.F32))
    t = O.conv2d(ctx, O.meanpool2(ctx, ctx.upload(x)), ws, FakeParam(ctx, P["bs"]).t, 1)
    ctx.sync()
    ctx.guard.check()
    return fused, ctx.view(t).view(torch.int16).clone()


def _oracle(mode, x, P):
    """float64 with the 16-bit rounding restated at the four points: h, xp, t, y."""
    q = lambda v: half_round(mode, v).astype(np.float64)
    x = x.astype(np.float64)
    wq = {k: q(P[k] / np.float32(SIGMA)) for k in ("ws", "w1", "w2")}
    h = q(nn.conv2d_fwd(x, wq["w1"]) + P["b1"])
    t = q(nn.conv2d_fwd(q(nn.meanpool2(x)), wq["ws"]) + P["bs"])
    return q(t + nn.meanpool2(nn.conv2d_fwd(np.maximum(h, 0), wq["w2"])) + P["b2"])


def _differ(a, b):
    return int((a != b).sum())


def _compare(ctx, mode, x, seed):
    P = _weights(seed)
    a, b = _block(ctx, x, P, True), _block(ctx, x, P, False)
    assert _differ(a["xp_bits"], b["xp_bits"]) == 0, "xp differs in %d elements" % _differ(a["xp_bits"], b["xp_bits"])
    assert _differ(a["h_bits"], b["h_bits"]) == 0, "h differs in %d elements" % _differ(a["h_bits"], b["h_bits"])
    tf, tu = _shortcut_bits(ctx, x, P)
    assert _differ(tf, tu) == 0, "t differs in %d elements" % _differ(tf, tu)
    print("%s: max |fused y - three launches| = %.3g" % (mode, float(np.abs(a["y"].astype(np.float64) - b["y"]).max())))
    assert_close(a["y"], b["y"], TOL[mode], "fused y vs three launches")
    assert_close(a["y"], _oracle(mode, x, P), 3 * TOL[mode], "fused y vs float64 restatement")


@pytest.mark.parametrize("n", [1, 3])
def test_fused_equals_three_launches(dev, n):
    """n = 1: four workgroups; n = 3: an odd grid.  Guard bands of every buffer untouched, no output element left unwritten (_block)."""
    ctx, mode = dev
    x = half_round(mode, np.random.RandomState(n).randn(n, 32, 32, 3))
    _compare(ctx, mode, x, n)


@pytest.mark.parametrize("kind", ["seam_rows", "frame"])
def test_band_seams_and_image_frame(dev, kind):
    """Inputs whose only support is rows 6..9, 14..17 and 22..25 (the rows of h two neighbouring bands both compute, and the input rows
    they need) or the image's frame (rows and columns 0 and 31: the clipped patch rows, the zero halo, the zero rows of relu(h))."""
    ctx, mode = dev
    full = np.random.RandomState(7).randn(2, 32, 32, 3)
    x = np.zeros_like(full)
    if kind == "seam_rows":
        for r0 in (6, 14, 22):
            x[:, r0:r0 + 4] = full[:, r0:r0 + 4]
    else:
        x[:, [0, 31]] = full[:, [0, 31]]
        x[:, :, [0, 31]] = full[:, :, [0, 31]]
    _compare(ctx, mode, half_round(mode, x), 11)


def test_given_pooled_images_are_not_stored(dev):
    """The critic step's pass: the pooled images exist (image_pool), the launch forms its own in LDS and stores none (_block checks)."""
    ctx, mode = dev
    x = half_round(mode, np.random.RandomState(5).randn(3, 32, 32, 3))
    P = _weights(5)
    a, b = _block(ctx, x, P, True, given_pool=True), _block(ctx, x, P, False, given_pool=True)
    assert _differ(a["h_bits"], b["h_bits"]) == 0 and _differ(a["xp_bits"], b["xp_bits"]) == 0
    assert_close(a["y"], b["y"], TOL[mode], "fused y vs three launches")
    # the shortcut from the launch's own pooled pixels equals the shortcut from the given ones: y has the bits of the pass that stores xp
    c = _block(ctx, x, P, True)
    assert _differ(a["y_bits"], c["y_bits"]) == 0


def test_stored_pooled_images_equal_meanpool2(dev):
    """The generator step's pass (x needs a gradient, no image_pool): xp is stored and has the bits of ops.meanpool2."""
    from rcgan_amd import ops as O
    ctx, mode = dev
    x = half_round(mode, np.random.RandomState(6).randn(3, 32, 32, 3))
    a = _block(ctx, x, _weights(6), True)
    ctx.new_step()
    ctx.guard.clear()
    ref = O.meanpool2(ctx, ctx.upload(x))
    ctx.sync()
    assert _differ(a["xp_bits"], ctx.view(ref).view(torch.int16)) == 0


def test_backward_is_unchanged(dev):
    """With x.req and a random dy the unchanged backward entries read dy, x, xp and h only, which are bit-equal: so are dx, the three
    filter gradients and the three bias gradients, at n = 3."""
    ctx, mode = dev
    n = 3
    rs = np.random.RandomState(33)
    x = half_round(mode, rs.randn(n, 32, 32, 3))
    dy = half_round(mode, rs.randn(n, 16, 16, 128))
    P = _weights(33)
    a, b = _block(ctx, x, P, True, dy), _block(ctx, x, P, False, dy)
    assert _differ(a["h_bits"], b["h_bits"]) == 0 and _differ(a["xp_bits"], b["xp_bits"]) == 0
    assert np.array_equal(a["dx"].view(np.uint32), b["dx"].view(np.uint32)), "dx"
    for k in ("ws", "w1", "w2"):
        assert np.array_equal(a["dw"][k].view(np.uint32), b["dw"][k].view(np.uint32)), k
    for k in ("bs", "b1", "b2"):
        assert np.array_equal(a["db"][k].view(np.uint32), b["db"][k].view(np.uint32)), k


def test_production_batch_has_the_three_launches_bits(dev):
    """n = 128 (512 workgroups, two rounds of one per CU): the three launches are the kernels of the training step (Conv2 on its gather form
    with ONE K group, K-tiles in order), and the fused kernel sums in their order: h, xp and y have their bits, so a training run through
    the fused forward computes what it computed through the three launches."""
    ctx, mode = dev
    n = 128
    x = half_round(mode, np.random.RandomState(128).randn(n, 32, 32, 3))
    P = _weights(128)
    a, b = _block(ctx, x, P, True, y_host=False), _block(ctx, x, P, False, y_host=False)
    assert _differ(a["xp_bits"], b["xp_bits"]) == 0 and _differ(a["h_bits"], b["h_bits"]) == 0
    differ = _differ(a["y_bits"], b["y_bits"])
    print("n = 128 %s: %d of %d elements of y differ in their bits" % (mode, differ, a["y_bits"].numel()))
    assert differ == 0, "y differs from the three launches in %d elements" % differ


def test_discriminator_takes_the_fused_block_or_the_three_launches(monkeypatch):
    """The CIFAR critic step calls ops.d_block1 by default; with the switch off rcgan_dblock1_ok is not asked, no copy is requested and the
    same step runs the three launches (ops.d_block1 is never entered, Conv1 and the shortcut go through ops.conv2d on the images)."""
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
        calls, image_convs, real, real_conv = [], [], O.d_block1, O.conv2d

        def conv2d(ctx, x, *a, **k):
            if x.shape[-1] == 3 and "_done" not in k:
                image_convs.append(tuple(x.shape))
            return real_conv(ctx, x, *a, **k)
        monkeypatch.setattr(O, "d_block1", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        monkeypatch.setattr(O, "conv2d", conv2d)
        cost_fused = m.eval_d_cost()
        assert len(calls) >= 1 and not image_convs, (calls, image_convs)
        assert m.graph.dblock1_frag is not None
        monkeypatch.setattr(O, "FUSED_DBLOCK1", False)
        seen = len(calls)
        cost_three = m.eval_d_cost()
        assert len(calls) == seen and m.graph.dblock1_frag is None
        assert {s[1] for s in image_convs} == {16, 32}, image_convs         # the shortcut on the pooled images, Conv1 on the images
        # (each evaluation moves the spectral norms' u vectors on, so the two costs are not the same number: the values are compared
        # at op level above and by the step tests, which now run through the fused forward)
        assert np.isfinite(cost_fused) and np.isfinite(cost_three), (cost_fused, cost_three)
    finally:
        m.ctx.close()
