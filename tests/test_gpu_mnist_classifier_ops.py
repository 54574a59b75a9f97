"""The two memory-bound operators of the MNIST label classifier (csrc/classifier.hip) bit for bit against tests/mnist_classifier_ref.py:
relu + 2x2 max pool with its first-maximum adjoint, and dropout on the device's Philox stream.  fp32 and both 16-bit formats; every
tensor a kernel reads or writes lives between guard bands (tests/guard.py), and every refused call leaves its outputs untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mnist_classifier_ref as R
from tests import philox_ref as P
from tests.gpu_util import half_round, make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

# (n, h, w, c): one window of one channel; odd channel count (scalar route everywhere); four channels (16 bytes in fp32); 12 channels
# (vector route in fp32, scalar in 16 bits) at a count that fills no whole block; the two production layers at batch 2 (vector routes)
POOL_SHAPES = [(1, 2, 2, 1), (3, 4, 6, 5), (1, 2, 2, 4), (5, 6, 10, 12), (2, 28, 28, 32), (2, 14, 14, 64)]
COUNTS = [1, 3, 4, 5, 1023, 128 * 1024]
KEEPS = [0.5, 0.9, 1.0]
SEED, START = (1 << 32) + 5, 1000


@pytest.fixture(scope="module")
def _contexts():
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx, arena_bytes=256 << 20, ws_bytes=1 << 20)
            ctx.guard = cm.__enter__()
            made[mode] = (ctx, cm)
        return made[mode][0], mode

    yield get
    for ctx, cm in made.values():
        cm.__exit__(None, None, None)
        ctx.close()


@pytest.fixture(scope="module", params=["f32", "bf16", "f16"])
def dev(request, _contexts):
    return _contexts(request.param)


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def _bytes(ctx, n):
    from rcgan_amd.runtime import DT
    return DT(ctx.arena.alloc(n), (n,), "u8", ctx.arena.buf)


def _get_bytes(ctx, t):
    off = t.ptr - t.base.data_ptr()
    with torch.cuda.stream(ctx.stream):
        out = t.base.view(torch.uint8).reshape(-1)[off:off + t.size].cpu()
    ctx.sync()
    return out.numpy()


def _fresh(ctx):
    ctx.guard.clear()
    ctx.new_step()


# ------------------------------------------------------------------------------------------------ relu + max pool
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_relu_maxpool2_is_selection_bit_for_bit(dev, shape):
    ctx, mode = dev
    g, dt = ctx.guard, ctx.act_dtype
    n, h, w, c = shape
    rs = np.random.RandomState(h * 100 + c)
    x = (rs.randint(-2, 3, size=shape) / 4.0).astype(np.float32)             # ties and zeros everywhere; exact in every format
    dy = half_round(mode, rs.randn(n, h // 2, w // 2, c).astype(np.float32))
    old = half_round(mode, rs.randn(*shape).astype(np.float32))
    _fresh(ctx)
    xd, dyd = ctx.upload(x, dt), ctx.upload(dy, dt)
    y = ctx.empty((n, h // 2, w // 2, c), dt)
    dx = ctx.empty(shape, dt)                                                 # starts out as NaN (the guard's fill): every element must be written
    dxa = ctx.upload(old, dt)
    ctx.check(ctx.lib.rcgan_relu_maxpool2_fwd(ctx.h, n, h, w, c, dt, _p(xd), _p(y)))
    ctx.check(ctx.lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, dt, _p(xd), _p(dyd), _p(dx), 0))
    ctx.check(ctx.lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, dt, _p(xd), _p(dyd), _p(dxa), 1))
    ctx.sync()
    g.check()
    assert g.unwritten(y) == 0 and g.unwritten(dx) == 0
    _same_bits(ctx.download(y), R.relu_maxpool2(x), "forward")
    contribution = R.relu_maxpool2_grad(x, dy)
    assert contribution.dtype == np.float32
    _same_bits(ctx.download(dx), contribution, "backward")
    _same_bits(ctx.download(dxa), half_round(mode, old + contribution), "backward, accumulate: the fp32 sum rounded once")
    _same_bits(ctx.download(xd), x, "the input")
    # every window hands its gradient to at most one element, and only where the output is positive
    assert (np.count_nonzero(R._windows(contribution), axis=-1) <= 1).all()
    assert (R._windows(contribution).sum(-1)[R.relu_maxpool2(x) <= 0] == 0).all()


def test_tape_ops(dev):
    """ops.relu_maxpool2 / ops.dropout: forward always, the closure only under recording, grad_of's destination and accumulate flag."""
    from rcgan_amd import ops as O
    ctx, mode = dev
    dt = ctx.act_dtype
    shape = (2, 4, 4, 8)
    rs = np.random.RandomState(5)
    x = (rs.randint(-2, 3, size=shape) / 4.0).astype(np.float32)
    dy = half_round(mode, rs.randn(2, 2, 2, 8).astype(np.float32))
    _fresh(ctx)
    with torch.cuda.stream(ctx.stream):
        state = torch.tensor([START, 0], dtype=torch.int64, device=ctx.device)
    ctx.recording = False
    try:
        xd = ctx.upload(x, dt)
        xd.req = True
        y = O.relu_maxpool2(ctx, xd)
        z = O.dropout(ctx, y, 0.5, SEED, state)
        assert not y.req and not z.req and ctx.tape == []
    finally:
        ctx.recording = True
    _same_bits(ctx.download(y), R.relu_maxpool2(x), "forward without a tape")
    mask0 = R.dropout_mask(SEED, START, y.size, 0.5).reshape(y.shape)
    _same_bits(ctx.download(z), np.where(mask0, R.relu_maxpool2(x) * np.float32(2), np.float32(0)), "dropout without a tape")
    y = O.relu_maxpool2(ctx, xd)
    z = O.dropout(ctx, y, 0.5, SEED, state)                      # the stream went on: the next quads
    assert y.req and z.req and len(ctx.tape) == 2
    z.grad = ctx.upload(dy, dt)
    ctx.backward()
    mask1 = R.dropout_mask(SEED, START + P.quads_of(y.size), y.size, 0.5).reshape(y.shape)
    assert (mask0 != mask1).any()
    dy_pool = np.where(mask1, dy * np.float32(2), np.float32(0)).astype(np.float32)
    _same_bits(ctx.download(y.grad), dy_pool, "dropout backward")
    first = R.relu_maxpool2_grad(x, dy_pool)
    _same_bits(ctx.download(xd.grad), first, "pool backward")
    # a second consumer adds to the gradient that is there
    y2 = O.relu_maxpool2(ctx, xd)
    y2.grad = ctx.upload(dy, dt)
    ctx.backward()
    _same_bits(ctx.download(xd.grad), half_round(mode, first + R.relu_maxpool2_grad(x, dy)), "pool backward, second consumer")
    ctx.sync()
    ctx.guard.check()
    assert state.tolist() == [START + 2 * P.quads_of(y.size), 0]


# ------------------------------------------------------------------------------------------------ dropout
@functools.lru_cache(maxsize=None)
def _units(count, first_quad):
    return P.unit24(P.stream_words(SEED, first_quad, count))


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("count", COUNTS)
def test_dropout_follows_the_stream_bit_for_bit(dev, count, keep):
    ctx, mode = dev
    g, dt = ctx.guard, ctx.act_dtype
    rs = np.random.RandomState(count % 1000 + int(keep * 10))
    x, dy, old = (half_round(mode, rs.randn(count).astype(np.float32)) for _ in range(3))
    _fresh(ctx)
    state = ctx.persistent((2,), "i32")
    ctx.upload(np.array([START, 0]), out=state)
    xd, dyd = ctx.upload(x, dt), ctx.upload(dy, dt)
    y, y2, dx, dxa = ctx.empty((count,), dt), ctx.empty((count,), dt), ctx.empty((count,), dt), ctx.upload(old, dt)
    mask, mask2 = _bytes(ctx, count), _bytes(ctx, count)
    ctx.check(ctx.lib.rcgan_dropout_fwd(ctx.h, count, dt, keep, SEED, _p(state), _p(xd), _p(y), _p(mask)))
    ctx.check(ctx.lib.rcgan_dropout_fwd(ctx.h, count, dt, keep, SEED, _p(state), _p(xd), _p(y2), _p(mask2)))
    ctx.check(ctx.lib.rcgan_dropout_bwd(ctx.h, count, dt, keep, _p(mask), _p(dyd), _p(dx), 0))
    ctx.check(ctx.lib.rcgan_dropout_bwd(ctx.h, count, dt, keep, _p(mask), _p(dyd), _p(dxa), 1))
    ctx.sync()
    g.check()
    for t in (y, y2, dx, mask, mask2):
        assert g.unwritten(t) == 0
    quads = P.quads_of(count)
    keep32, scale = np.float32(keep), R.dropout_scale(keep)
    want, want2 = _units(count, START) < keep32, _units(count, START + quads) < keep32
    assert (want == R.dropout_mask(SEED, START, count, keep)).all()
    got = _get_bytes(ctx, mask)
    assert (got == want.astype(np.uint8)).all(), "mask: %d of %d differ" % (int((got != want).sum()), count)
    assert (_get_bytes(ctx, mask2) == want2.astype(np.uint8)).all(), "the second call draws the next quads"
    if keep == 1.0:
        assert want.all() and float(scale) == 1.0
    zero = np.float32(0)
    _same_bits(ctx.download(y), half_round(mode, np.where(want, x * scale, zero)), "y")
    _same_bits(ctx.download(y2), half_round(mode, np.where(want2, x * scale, zero)), "y of the second call")
    assert ctx.download(state).tolist() == [START + 2 * quads, 0]
    contribution = np.where(want, dy * scale, zero).astype(np.float32)
    _same_bits(ctx.download(dx), half_round(mode, contribution), "backward")
    _same_bits(ctx.download(dxa), half_round(mode, old + contribution), "backward, accumulate")
    _same_bits(ctx.download(xd), x, "the input")


def test_dropout_without_a_state_starts_at_offset_zero(dev):
    ctx, mode = dev
    dt, count = ctx.act_dtype, 37
    x = half_round(mode, np.random.RandomState(1).randn(count).astype(np.float32))
    _fresh(ctx)
    xd, y, mask = ctx.upload(x, dt), ctx.empty((count,), dt), _bytes(ctx, count)
    ctx.check(ctx.lib.rcgan_dropout_fwd(ctx.h, count, dt, 0.5, SEED, None, _p(xd), _p(y), _p(mask)))
    ctx.sync()
    ctx.guard.check()
    want = R.dropout_mask(SEED, 0, count, 0.5)
    assert (_get_bytes(ctx, mask) == want).all()
    _same_bits(ctx.download(y), np.where(want, x * np.float32(2), np.float32(0)), "y")


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_are_refused_before_anything_is_launched(dev):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    g, dt = ctx.guard, ctx.act_dtype
    other16 = L.BF16 if dt == L.F16 else L.F16 if dt == L.BF16 else None      # the 16-bit type of the OTHER build is unknown to this one
    lib = ctx.lib
    _fresh(ctx)
    n, h, w, c = 2, 4, 4, 8
    x, dy = ctx.empty((n, h, w, c), dt), ctx.empty((n, h // 2, w // 2, c), dt)
    y, dx = ctx.empty((n, h // 2, w // 2, c), dt), ctx.empty((n, h, w, c), dt)
    count = n * h * w * c
    mask = _bytes(ctx, count)
    state = ctx.persistent((2,), "i32")
    ctx.upload(np.array([START, 0]), out=state)
    X, DY, Y, DX, M, S = _p(x), _p(dy), _p(y), _p(dx), _p(mask), _p(state)
    bad_dtypes = [7, -1] + ([other16] if other16 is not None and mode != "f32" else [])
    if mode == "f32":
        bad_dtypes.append(L.F16)                                               # the default build's 16-bit type is bf16
    calls = []
    for shp in [(0, h, w, c), (n, 0, w, c), (n, h, 0, c), (n, h, w, 0), (-1, h, w, c), (n, 3, w, c), (n, h, 5, c), (n, 1, 1, c)]:
        calls.append(("pool fwd %r" % (shp,), lambda s=shp: lib.rcgan_relu_maxpool2_fwd(ctx.h, s[0], s[1], s[2], s[3], dt, X, Y)))
        calls.append(("pool bwd %r" % (shp,), lambda s=shp: lib.rcgan_relu_maxpool2_bwd(ctx.h, s[0], s[1], s[2], s[3], dt, X, DY, DX, 0)))
    calls += [("pool fwd NULL x", lambda: lib.rcgan_relu_maxpool2_fwd(ctx.h, n, h, w, c, dt, None, Y)),
              ("pool fwd NULL y", lambda: lib.rcgan_relu_maxpool2_fwd(ctx.h, n, h, w, c, dt, X, None)),
              ("pool bwd NULL x", lambda: lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, dt, None, DY, DX, 0)),
              ("pool bwd NULL dy", lambda: lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, dt, X, None, DX, 1)),
              ("pool bwd NULL dx", lambda: lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, dt, X, DY, None, 0)),
              ("dropout fwd count 0", lambda: lib.rcgan_dropout_fwd(ctx.h, 0, dt, 0.5, SEED, S, X, DX, M)),
              ("dropout bwd count 0", lambda: lib.rcgan_dropout_bwd(ctx.h, 0, dt, 0.5, M, X, DX, 0)),
              ("dropout fwd NULL x", lambda: lib.rcgan_dropout_fwd(ctx.h, count, dt, 0.5, SEED, S, None, DX, M)),
              ("dropout fwd NULL y", lambda: lib.rcgan_dropout_fwd(ctx.h, count, dt, 0.5, SEED, S, X, None, M)),
              ("dropout fwd NULL mask", lambda: lib.rcgan_dropout_fwd(ctx.h, count, dt, 0.5, SEED, S, X, DX, None)),
              ("dropout bwd NULL mask", lambda: lib.rcgan_dropout_bwd(ctx.h, count, dt, 0.5, None, X, DX, 0)),
              ("dropout bwd NULL dy", lambda: lib.rcgan_dropout_bwd(ctx.h, count, dt, 0.5, M, None, DX, 1)),
              ("dropout bwd NULL dx", lambda: lib.rcgan_dropout_bwd(ctx.h, count, dt, 0.5, M, X, None, 0))]
    for kp in (0.0, -0.5, 1.0000001, 1.5, float("nan"), float("inf"), float("-inf")):
        calls.append(("dropout fwd keep_prob %r" % kp, lambda k=kp: lib.rcgan_dropout_fwd(ctx.h, count, dt, k, SEED, S, X, DX, M)))
        calls.append(("dropout bwd keep_prob %r" % kp, lambda k=kp: lib.rcgan_dropout_bwd(ctx.h, count, dt, k, M, X, DX, 0)))
    for bd in bad_dtypes:
        calls += [("pool fwd dtype %d" % bd, lambda d=bd: lib.rcgan_relu_maxpool2_fwd(ctx.h, n, h, w, c, d, X, Y)),
                  ("pool bwd dtype %d" % bd, lambda d=bd: lib.rcgan_relu_maxpool2_bwd(ctx.h, n, h, w, c, d, X, DY, DX, 0)),
                  ("dropout fwd dtype %d" % bd, lambda d=bd: lib.rcgan_dropout_fwd(ctx.h, count, d, 0.5, SEED, S, X, DX, M)),
                  ("dropout bwd dtype %d" % bd, lambda d=bd: lib.rcgan_dropout_bwd(ctx.h, count, d, 0.5, M, X, DX, 0))]
    for what, call in calls:
        rc = call()
        assert rc == L.EINVALID_ARG, "%s returned %d" % (what, rc)
        assert lib.rcgan_last_error(ctx.h)
    ctx.sync()
    g.check()
    for t in (x, dy, y, dx, mask):
        assert g.unwritten(t) == t.size, "a refused call wrote to a buffer"
    assert ctx.download(state).tolist() == [START, 0], "a refused call advanced the stream"
