"""The elementwise, resampling and random-number kernels (csrc/elementwise.hip, csrc/rng.h) on the routes production takes, called
through the C ABI on torch buffers placed by the test: the 8-channel vector resampling kernel next to its scalar fallbacks, every
``accumulate`` switch from a non-zero destination, the grid-stride wrap of both grid caps, casts and copies bit for bit, and
rcgan_rng_fill word for word against tests/philox_ref.py.  Every output sits between two sentinel margins that must come back
untouched.  Tolerances are those of test_gpu_ops.py (inputs pre-rounded to the 16-bit format, one rounding of the stored result)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nn
from tests import philox_ref as P
from tests.gpu_util import HALF, assert_close, half_round, make_ctx

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 1e-2, "f16": 3e-3}     # test_gpu_ops.py
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MARGIN = 256                                       # bytes of sentinel on either side of an output (keeps it 256-byte aligned)
SENTINEL = 0xA5


@pytest.fixture(scope="module", params=["f32", "bf16", "f16"])
def dev(request):
    ctx = make_ctx(request.param, arena=1 << 24)
    yield ctx, request.param
    ctx.close()


def _code(mode):
    from rcgan_amd import _lib as L
    return {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}[mode]


def _half_mode(mode):
    """The 16-bit format of the library that serves ``mode`` (the bf16 library serves f32)."""
    return "f16" if mode == "f16" else "bf16"


class Out:
    """An output buffer of ``shape`` between two sentinel margins; ``shift`` bytes move it off its 256-byte alignment."""

    def __init__(self, ctx, shape, tdt, init=None, shift=0):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=tdt).element_size()
        self.raw = torch.full((MARGIN + shift + nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        self.lo, self.hi = MARGIN + shift, MARGIN + shift + nbytes
        self.t = self.raw[self.lo:self.hi].view(tdt).reshape(shape)
        self.ptr = C.c_void_p(self.raw.data_ptr() + self.lo)
        if init is None:
            if tdt.is_floating_point:
                self.t.fill_(float("nan"))          # an entry that must not read its destination would carry this through
        else:
            self.t.copy_(init if isinstance(init, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(init)))

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())

    def np(self):
        assert self.intact(), "a sentinel margin was overwritten"
        return (self.t.float() if self.t.dtype.is_floating_point else self.t).cpu().numpy()


def _dev(ctx, arr, tdt):
    """numpy -> device tensor of dtype tdt (float arrays are already rounded to it: the conversion is exact)."""
    return torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device).to(tdt).contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _call(ctx, fn, *args):
    """One library call between two synchronisations: the torch work before it ran on another stream.  Tensors among ``args`` go in
    as their addresses and stay alive until the call has finished (a temporary freed earlier would hand its memory to the next one)."""
    torch.cuda.synchronize()
    ctx.check(fn(ctx.h, *[_p(a) if isinstance(a, torch.Tensor) else a for a in args]))
    ctx.sync()


def _rand(rs, shape, mode):
    return half_round(mode, rs.randn(*shape).astype(np.float32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ------------------------------------------------------------------------------------------------ resampling, both routes
# (n, low-resolution rows, columns, channels): c % 8 == 0 takes resample2_vec_kernel with 1 / 3 / 8 chunks per pixel, the others the
# scalar kernels; the 3 x 5 grid is non-square and odd
RESAMPLE = [(3, 3, 5, 8), (3, 3, 5, 24), (3, 3, 5, 64), (3, 3, 5, 10), (3, 3, 5, 12), (3, 1, 1, 8)]


def _meanpool_f32(x):
    """(((a00 + a10) + a01) + a11) * 0.25f in float32: the add_n order of the reference model, no product that could be fused."""
    x = np.asarray(x, np.float32)
    s = ((x[:, ::2, ::2] + x[:, 1::2, ::2]) + x[:, ::2, 1::2]) + x[:, 1::2, 1::2]
    assert s.dtype == np.float32
    return s * np.float32(0.25)


@pytest.mark.parametrize("shape", RESAMPLE)
def test_meanpool2_fwd(dev, shape):
    ctx, mode = dev
    n, oh, ow, c = shape
    x = _rand(np.random.RandomState(sum(shape)), (n, 2 * oh, 2 * ow, c), mode)
    y = Out(ctx, (n, oh, ow, c), TDT[mode])
    _call(ctx, ctx.lib.rcgan_meanpool2_fwd, n, 2 * oh, 2 * ow, c, _code(mode), _dev(ctx, x, TDT[mode]), y.ptr)
    got = y.np()
    assert_close(got, nn.meanpool2(x.astype(np.float64)), TOL[mode], "meanpool fwd %s" % (shape,))
    # the fixed-order float32 sum, rounded once (the step-input rider reproduces these values: csrc/step_inputs.h)
    _assert_bits(got, half_round(mode, _meanpool_f32(x)), "meanpool fwd order %s" % (shape,))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", RESAMPLE)
def test_meanpool2_bwd(dev, shape, accumulate):
    ctx, mode = dev
    n, oh, ow, c = shape
    rs = np.random.RandomState(sum(shape) + 100)
    dy = _rand(rs, (n, oh, ow, c), mode)
    prev = _rand(rs, (n, 2 * oh, 2 * ow, c), mode)
    dx = Out(ctx, prev.shape, TDT[mode], init=_dev(ctx, prev, TDT[mode]) if accumulate else None)
    _call(ctx, ctx.lib.rcgan_meanpool2_bwd, n, 2 * oh, 2 * ow, c, _code(mode), _dev(ctx, dy, TDT[mode]), dx.ptr, accumulate)
    ref = nn.meanpool2_bwd(dy.astype(np.float64)) + (prev if accumulate else 0.0)
    assert_close(dx.np(), ref, TOL[mode], "meanpool bwd %s acc %d" % (shape, accumulate))


@pytest.mark.parametrize("shape", RESAMPLE)
def test_upsample2_fwd(dev, shape):
    ctx, mode = dev
    n, oh, ow, c = shape
    x = _rand(np.random.RandomState(sum(shape) + 200), (n, oh, ow, c), mode)
    y = Out(ctx, (n, 2 * oh, 2 * ow, c), TDT[mode])
    _call(ctx, ctx.lib.rcgan_upsample2_fwd, n, 2 * oh, 2 * ow, c, _code(mode), _dev(ctx, x, TDT[mode]), y.ptr)
    _assert_bits(y.np(), nn.upsample2(x), "upsample fwd %s" % (shape,))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", RESAMPLE)
def test_upsample2_bwd(dev, shape, accumulate):
    ctx, mode = dev
    n, oh, ow, c = shape
    rs = np.random.RandomState(sum(shape) + 300)
    dy = _rand(rs, (n, 2 * oh, 2 * ow, c), mode)
    prev = _rand(rs, (n, oh, ow, c), mode)
    dx = Out(ctx, prev.shape, TDT[mode], init=_dev(ctx, prev, TDT[mode]) if accumulate else None)
    _call(ctx, ctx.lib.rcgan_upsample2_bwd, n, 2 * oh, 2 * ow, c, _code(mode), _dev(ctx, dy, TDT[mode]), dx.ptr, accumulate)
    ref = nn.upsample2_bwd(dy.astype(np.float64)) + (prev if accumulate else 0.0)
    assert_close(dx.np(), ref, TOL[mode], "upsample bwd %s acc %d" % (shape, accumulate))


# ------------------------------------------------------------------------------------------------ grid-stride wrap, one case per cap
def test_act_fwd_past_the_grid_cap(dev):
    """ew_grid stops at 8192 workgroups of 256 threads: 2^21 + 12345 elements make every thread take a second element or not."""
    from rcgan_amd import _lib as L
    ctx, _ = dev
    count = (1 << 21) + 12345
    x = torch.randn(count, device=ctx.device)
    y = Out(ctx, (count,), torch.float32)
    _call(ctx, ctx.lib.rcgan_act_fwd, count, L.F32, L.ACT_LRELU, _p(x), y.ptr)
    assert y.intact()
    assert torch.equal(y.t, torch.maximum(x, x * 0.2))


def test_resample_past_the_grid_cap(dev):
    """resample_grid stops at 16384 workgroups of 256 chunks: [66, 128, 128, 32] low-resolution pixels are 4 325 376 chunks of eight
    16-bit channels.  Both expected tensors are exact (replication; the fixed-order float32 sum rounded once) and built on the device."""
    ctx, mode = dev
    if mode not in HALF:
        pytest.skip("the bf16 mode runs the 16-bit kernel of the same library")
    n, oh, ow, c = 66, 128, 128, 32
    assert n * oh * ow * c // 8 > 16384 * 256
    tdt = TDT[mode]
    try:
        hi = torch.randn(n, 2 * oh, 2 * ow, c, device=ctx.device).to(tdt)
        low = Out(ctx, (n, oh, ow, c), tdt)
        _call(ctx, ctx.lib.rcgan_meanpool2_fwd, n, 2 * oh, 2 * ow, c, _code(mode), _p(hi), low.ptr)
        f = lambda i, j: hi[:, i::2, j::2].float()
        want = ((((f(0, 0) + f(1, 0)) + f(0, 1)) + f(1, 1)) * 0.25).to(tdt)
        assert low.intact() and torch.equal(low.t, want)
        del want, f
        src = low.t.clone()
        out = Out(ctx, (n, 2 * oh, 2 * ow, c), tdt, init=hi)       # (not NaN: torch.equal below)
        del hi
        _call(ctx, ctx.lib.rcgan_upsample2_fwd, n, 2 * oh, 2 * ow, c, _code(mode), _p(src), out.ptr)
        assert out.intact()
        for i in (0, 1):
            for j in (0, 1):
                assert torch.equal(out.t[:, i::2, j::2], src), (i, j)
    finally:
        hi = low = out = src = want = f = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ plain elementwise
COUNT = 1027        # odd, five workgroups


def _act_ref(act, x):
    from rcgan_amd import _lib as L
    x = x.astype(np.float64)
    return {L.ACT_NONE: lambda: x, L.ACT_RELU: lambda: np.where(x > 0, x, 0.0), L.ACT_LRELU: lambda: np.maximum(x, 0.2 * x),
            L.ACT_TANH: lambda: np.tanh(x), L.ACT_SIGMOID: lambda: 1 / (1 + np.exp(-x))}[act]()


def _act_grad_ref(act, s):
    from rcgan_amd import _lib as L
    s = s.astype(np.float64)
    return {L.ACT_NONE: lambda: np.ones_like(s), L.ACT_RELU: lambda: np.where(s > 0, 1.0, 0.0), L.ACT_LRELU: lambda: np.where(s > 0, 1.0, 0.2),
            L.ACT_TANH: lambda: 1 - s * s, L.ACT_SIGMOID: lambda: s * (1 - s)}[act]()


def _act_input(mode, seed):
    x = _rand(np.random.RandomState(seed), (COUNT,), mode)
    x[:6] = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0]        # the mask is x > 0: both zeros are outside it
    return x


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_act_fwd(dev, act):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    assert sorted((L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SIGMOID)) == [0, 1, 2, 3, 4]
    x = _act_input(mode, 10 + act)
    y = Out(ctx, (COUNT,), TDT[mode])
    _call(ctx, ctx.lib.rcgan_act_fwd, COUNT, _code(mode), act, _dev(ctx, x, TDT[mode]), y.ptr)
    got = y.np()
    assert_close(got, _act_ref(act, x), TOL[mode], "act fwd %d" % act)
    if act == L.ACT_NONE:
        _assert_bits(got, x, "act none")
    if act == L.ACT_RELU:
        assert np.array_equal(got, np.where(x > 0, x, np.float32(0))) and not np.signbit(got[:4]).any()
    if act == L.ACT_LRELU:
        assert (got[:4] == 0).all()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_act_bwd(dev, act, accumulate):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(20 + act)
    x = _act_input(mode, 10 + act)
    # relu / lrelu take the pre-activation x, tanh / sigmoid their own (stored, rounded) output
    s = half_round(mode, _act_ref(act, x)) if act in (L.ACT_TANH, L.ACT_SIGMOID) else x
    dy, prev = _rand(rs, (COUNT,), mode), _rand(rs, (COUNT,), mode)
    dx = Out(ctx, (COUNT,), TDT[mode], init=_dev(ctx, prev, TDT[mode]) if accumulate else None)
    _call(ctx, ctx.lib.rcgan_act_bwd, COUNT, _code(mode), act, _dev(ctx, s, TDT[mode]), _dev(ctx, dy, TDT[mode]), dx.ptr, accumulate)
    got = dx.np()
    assert_close(got, dy * _act_grad_ref(act, s) + (prev if accumulate else 0.0), TOL[mode], "act bwd %d acc %d" % (act, accumulate))
    if not accumulate and act in (L.ACT_NONE, L.ACT_RELU):
        assert np.array_equal(got, dy if act == L.ACT_NONE else np.where(x > 0, dy, np.float32(0))), "act bwd mask %d" % act
    if not accumulate and act == L.ACT_LRELU:
        assert np.array_equal(got[x > 0], dy[x > 0])
        assert_close(got[:4], 0.2 * dy[:4].astype(np.float64), TOL[mode], "lrelu slope at +-0")


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (-0.25, 1.0), (2.0, 0.5)])
def test_axpby(dev, alpha, beta):
    ctx, mode = dev
    rs = np.random.RandomState(31)
    a, y0 = _rand(rs, (COUNT,), mode), _rand(rs, (COUNT,), mode)
    y = Out(ctx, (COUNT,), TDT[mode], init=_dev(ctx, y0, TDT[mode]))
    _call(ctx, ctx.lib.rcgan_axpby, COUNT, _code(mode), alpha, _dev(ctx, a, TDT[mode]), beta, y.ptr)
    assert_close(y.np(), alpha * a.astype(np.float64) + beta * y0.astype(np.float64), TOL[mode], "axpby %g %g" % (alpha, beta))


def test_axpby_beta_zero_does_not_read_y(dev):
    """ops.py hands rcgan_axpby(1, a, 0, y) a fresh, uninitialised y."""
    ctx, mode = dev
    a = _rand(np.random.RandomState(32), (COUNT,), mode)
    y = Out(ctx, (COUNT,), TDT[mode])          # NaN
    assert bool(torch.isnan(y.t).all())
    _call(ctx, ctx.lib.rcgan_axpby, COUNT, _code(mode), 1.0, _dev(ctx, a, TDT[mode]), 0.0, y.ptr)
    got = y.np()
    assert np.isfinite(got).all()
    _assert_bits(got, a, "axpby(1, a, 0, NaN)")


def test_add(dev):
    ctx, mode = dev
    rs = np.random.RandomState(33)
    a, b = _rand(rs, (COUNT,), mode), _rand(rs, (COUNT,), mode)
    y = Out(ctx, (COUNT,), TDT[mode])
    _call(ctx, ctx.lib.rcgan_add, COUNT, _code(mode), _dev(ctx, a, TDT[mode]), _dev(ctx, b, TDT[mode]), y.ptr)
    got = y.np()
    assert_close(got, a.astype(np.float64) + b, TOL[mode], "add")
    _assert_bits(got, half_round(mode, a + b), "add: one rounding of the float32 sum")


def _cast_input(half):
    """float32 values whose 16-bit rounding is delicate: exact ties (to even both ways), the largest finite values, a value that
    overflows fp16, subnormals of either format, +-0, +-inf, NaN, and a sweep over the exponent range."""
    e = 2.0 ** -8 if half == "bf16" else 2.0 ** -11          # half an ulp of 1.0 in the 16-bit format
    v = [1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 1 + e * (1 + 2.0 ** -10), 1 + e * (1 - 2.0 ** -10),
         3.4028235e38, -3.4028235e38, 3.3895314e38, 3.3961775e38, 65504.0, 65519.996, 65520.0, 1e5, -1e5,
         1e-45, -1e-45, 1e-40, 9.18355e-41, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 6e-8, 6.1e-5, 2.0 ** -14,
         1.1754944e-38, 0.0, -0.0, np.inf, -np.inf, np.nan]
    rs = np.random.RandomState(41)
    sweep = rs.randn(COUNT - len(v)) * np.exp2(rs.randint(-40, 40, size=COUNT - len(v)))
    with np.errstate(over="ignore"):
        return np.concatenate([np.array(v, np.float64), sweep]).astype(np.float32)


def test_cast(dev):
    """All four dtype pairs of rcgan_cast.  f32 -> 16-bit is torch's round-to-nearest-even bit for bit; 16-bit -> f32 is exact over
    ALL 65536 patterns; NaN stays NaN (its payload is not compared)."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    half = _half_mode(mode)
    hdt, hcode = TDT[half], _code(half)
    x = _cast_input(half)
    xd = _dev(ctx, x, torch.float32)
    want16 = torch.from_numpy(x).to(hdt)                       # CPU conversion: round to nearest even
    nan = np.isnan(x)
    y = Out(ctx, (COUNT,), hdt)
    _call(ctx, ctx.lib.rcgan_cast, COUNT, L.F32, _p(xd), hcode, y.ptr)
    assert y.intact()
    got16 = y.t.cpu()
    assert bool(torch.isnan(got16[torch.from_numpy(nan)]).all())
    g, w = got16.view(torch.int16).numpy()[~nan], want16.view(torch.int16).numpy()[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "f32 -> %s: %r -> %#x, want %#x" % (half, x[~nan][bad[0]], g[bad[0]] & 0xffff, w[bad[0]] & 0xffff)
    # 16-bit -> f32 and 16-bit -> 16-bit over every pattern
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(hdt)
    pd = pat.to(ctx.device)
    pnan = torch.isnan(pat).numpy()
    z = Out(ctx, (65536,), torch.float32)
    _call(ctx, ctx.lib.rcgan_cast, 65536, hcode, _p(pd), L.F32, z.ptr)
    got = z.np()
    assert np.isnan(got[pnan]).all()
    _assert_bits(got[~pnan], pat.float().numpy()[~pnan], "%s -> f32" % half)
    h = Out(ctx, (65536,), hdt)
    _call(ctx, ctx.lib.rcgan_cast, 65536, hcode, _p(pd), hcode, h.ptr)
    assert h.intact()
    goth = h.t.cpu()
    assert bool(torch.isnan(goth[torch.from_numpy(pnan)]).all())
    assert np.array_equal(goth.view(torch.int16).numpy()[~pnan], pat.view(torch.int16).numpy()[~pnan])
    f = Out(ctx, (COUNT,), torch.float32)
    _call(ctx, ctx.lib.rcgan_cast, COUNT, L.F32, _p(xd), L.F32, f.ptr)
    got = f.np()
    assert np.isnan(got[nan]).all()
    _assert_bits(got[~nan], x[~nan], "f32 -> f32")


@pytest.mark.parametrize("count", [0, 1, COUNT])
def test_fill_f32(dev, count):
    ctx, _ = dev
    y = Out(ctx, (count,), torch.float32)
    _call(ctx, ctx.lib.rcgan_fill_f32, count, y.ptr, -1.5)
    assert np.array_equal(y.np(), np.full(count, -1.5, np.float32))


@pytest.mark.parametrize("shifts", [(0, 0), (4, 0), (0, 4)], ids=["aligned", "src+4", "dst+4"])
@pytest.mark.parametrize("count", [1, 3, 4, 7, COUNT])
def test_copy_words(dev, count, shifts):
    """16-byte pieces where both sides are 16-byte aligned and a word tail; words alone when either side is not."""
    ctx, _ = dev
    words = torch.from_numpy(np.random.RandomState(count).randint(-2 ** 31, 2 ** 31, size=count, dtype=np.int64).astype(np.int32))
    src = Out(ctx, (count,), torch.int32, init=words, shift=shifts[0])
    dst = Out(ctx, (count,), torch.int32, shift=shifts[1])
    assert src.ptr.value % 16 == shifts[0] and dst.ptr.value % 16 == shifts[1]
    _call(ctx, ctx.lib.rcgan_copy_words, count, src.ptr, dst.ptr)
    assert np.array_equal(dst.np(), words.numpy()) and src.intact()


@pytest.mark.parametrize("before,c,after", [(0, 5, 3), (4, 8, 4), (3, 1, 0)])
def test_pad_channels(dev, before, c, after):
    ctx, mode = dev
    rows = 37
    x = _rand(np.random.RandomState(50 + c), (rows, c), mode)
    y = Out(ctx, (rows, before + c + after), TDT[mode])
    _call(ctx, ctx.lib.rcgan_pad_channels, rows, c, before, after, _code(mode), _dev(ctx, x, TDT[mode]), y.ptr)
    _assert_bits(y.np(), np.pad(x, ((0, 0), (before, after))), "pad channels")


@pytest.mark.parametrize("c1,c2", [(10, 10), (8, 3), (1, 16)])
def test_concat_channels(dev, c1, c2):
    ctx, mode = dev
    n, hw = 3, 6
    rs = np.random.RandomState(60 + c1)
    x, yb = _rand(rs, (n, hw, c1), mode), _rand(rs, (n, c2), mode)           # (label rows are fp32 in memory; pre-rounded values)
    y = Out(ctx, (n, hw, c1 + c2), TDT[mode])
    _call(ctx, ctx.lib.rcgan_concat_channels_fwd, n, hw, c1, c2, _code(mode), _dev(ctx, x, TDT[mode]), _dev(ctx, yb, torch.float32), y.ptr)
    _assert_bits(y.np(), np.concatenate([x, np.broadcast_to(yb[:, None, :], (n, hw, c2))], axis=2), "concat fwd")
    dy = _rand(rs, (n, hw, c1 + c2), mode)
    dx = Out(ctx, (n, hw, c1), TDT[mode])
    _call(ctx, ctx.lib.rcgan_concat_channels_bwd, n, hw, c1, c2, _code(mode), _dev(ctx, dy, TDT[mode]), dx.ptr)
    _assert_bits(dx.np(), dy[..., :c1], "concat bwd")


@pytest.mark.parametrize("reps", [1, 10])
def test_tile_rows_fwd(dev, reps):
    ctx, mode = dev
    x = _rand(np.random.RandomState(70), (COUNT,), mode)
    y = Out(ctx, (reps, COUNT), TDT[mode])
    _call(ctx, ctx.lib.rcgan_tile_rows_fwd, COUNT, reps, _code(mode), _dev(ctx, x, TDT[mode]), y.ptr)
    _assert_bits(y.np(), np.tile(x, (reps, 1)), "tile rows fwd")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("reps", [1, 10])
def test_tile_rows_bwd(dev, reps, accumulate):
    """dx (+)= sum_r dy[r]: a float32 sum in the order previous value, r = 0, 1, ..., rounded once (include/rcgan_hip.h)."""
    ctx, mode = dev
    rs = np.random.RandomState(71 + reps)
    dy, prev = _rand(rs, (reps, COUNT), mode), _rand(rs, (COUNT,), mode)
    dx = Out(ctx, (COUNT,), TDT[mode], init=_dev(ctx, prev, TDT[mode]) if accumulate else None)
    _call(ctx, ctx.lib.rcgan_tile_rows_bwd, COUNT, reps, _code(mode), _dev(ctx, dy, TDT[mode]), dx.ptr, accumulate)
    s = prev.copy() if accumulate else np.zeros(COUNT, np.float32)
    for r in range(reps):
        s = s + dy[r]
    assert s.dtype == np.float32
    got = dx.np()
    assert_close(got, dy.astype(np.float64).sum(0) + (prev if accumulate else 0.0), TOL[mode], "tile rows bwd")
    _assert_bits(got, half_round(mode, s), "tile rows bwd: float32 sum rounded once")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,cols", [(10, 37), (1, 5), (5, 1)])
def test_transpose_f32(dev, rows, cols, accumulate):
    ctx, _ = dev
    rs = np.random.RandomState(80 + rows)
    x, prev = rs.randn(rows, cols).astype(np.float32), rs.randn(cols, rows).astype(np.float32)
    y = Out(ctx, (cols, rows), torch.float32, init=prev if accumulate else None)
    _call(ctx, ctx.lib.rcgan_transpose_f32, rows, cols, _dev(ctx, x, torch.float32), y.ptr, accumulate)
    _assert_bits(y.np(), prev + x.T if accumulate else x.T, "transpose")


# ------------------------------------------------------------------------------------------------ rcgan_rng_fill
def _state(ctx, value):
    return torch.tensor([value, 0], dtype=torch.int64, device=ctx.device)


def _draw(ctx, count, mode, kind, lo, hi, seed, state, first=None):
    """One guarded draw -> float32 numpy.  ``state``: None (offset 0) or a device tensor (advanced by the call)."""
    y = Out(ctx, (count,), TDT[mode])
    _call(ctx, ctx.lib.rcgan_rng_fill, count, _code(mode), kind, lo, hi, seed, _p(state) if state is not None else None, y.ptr)
    return y.np()


def test_rng_words(dev):
    """Uniform (0, 1) in f32 is (r >> 8) * 2^-24 exactly: the 24 bits used of every word, for draws that end inside a quad, offsets
    across the carry into the high counter word, and seeds whose high half matters; the state moves by ceil(count / 4)."""
    ctx, _ = dev
    for seed in (1234, (1 << 32) + 5, (1 << 63) + 1):
        for start in (None, 7, (1 << 32) - 2):
            for count in (1, 3, 4, 5, 4099):
                st = None if start is None else _state(ctx, start)
                got = _draw(ctx, count, "f32", 0, 0.0, 1.0, seed, st)
                want = P.unit24(P.stream_words(seed, start or 0, count))
                _assert_bits(got, want, "words seed %#x start %r count %d" % (seed, start, count))
                if st is not None:
                    assert st.tolist() == [start + P.quads_of(count), 0], (seed, start, count, st.tolist())


def test_rng_state_continues(dev):
    ctx, _ = dev
    seed, start = 99, 1000
    words = lambda q, count: P.unit24(P.stream_words(seed, start + q, count))
    draw = lambda st, count: _draw(ctx, count, "f32", 0, 0.0, 1.0, seed, st)
    st = _state(ctx, start)
    a, b = draw(st, 8), draw(st, 12)
    st2 = _state(ctx, start)
    _assert_bits(np.concatenate([a, b]), draw(st2, 20), "8 + 12 against 20")
    _assert_bits(np.concatenate([a, b]), words(0, 20), "8 + 12 against the reference")
    assert st.tolist() == st2.tolist() == [start + 5, 0]
    st = _state(ctx, start)
    a, b = draw(st, 5), draw(st, 12)
    _assert_bits(a, words(0, 5), "a cut quad")
    _assert_bits(b, words(2, 12), "the draw after a cut quad starts at the next quad")
    assert st.tolist() == [start + 5, 0]


def test_rng_graph_replays_walk_the_stream(dev):
    """A captured draw replayed twice returns the next two segments of the stream."""
    ctx, _ = dev
    seed, start, count = 4321, (1 << 32) - 3, 10
    st = _state(ctx, start)
    y = Out(ctx, (count,), torch.float32)
    from rcgan_amd import _lib as L
    fill = lambda: ctx.check(ctx.lib.rcgan_rng_fill(ctx.h, count, L.F32, 0, 0.0, 1.0, seed, _p(st), y.ptr))
    seg = lambda i: P.unit24(P.stream_words(seed, start + 3 * i, count))
    torch.cuda.synchronize()
    fill()
    ctx.sync()
    _assert_bits(y.np(), seg(0), "eager draw")
    ctx.graph_begin()
    fill()
    gid = ctx.graph_end()
    try:
        for i in (1, 2):
            ctx.graph_launch(gid)
            ctx.sync()
            _assert_bits(y.np(), seg(i), "replay %d" % i)
        assert st.tolist() == [start + 9, 0]
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))


def _h16_neighbour(mode, x, up):
    """The next value of the 16-bit format above / below the (representable) x."""
    x = np.float32(x)
    if mode == "f16":
        return np.float32(np.nextafter(np.float16(x), np.float16(np.inf if up else -np.inf)))
    b = int(x.view(np.uint32)) >> 16
    if b & 0x7fff == 0:
        b = 0x0001 if up else 0x8001
    else:
        b = b + 1 if bool(b & 0x8000) != up else b - 1
    return np.array([b << 16], np.uint32).view(np.float32)[0]


def _stored_range(mode, lo, hi):
    """[smallest value >= lo, largest value < hi] of the output format."""
    lo, hi = np.float32(lo), np.float32(hi)
    if mode == "f32":
        return lo, P.below(hi)
    a, b = np.float32(half_round(mode, lo)), np.float32(half_round(mode, hi))
    if a < lo:
        a = _h16_neighbour(mode, a, True)
    if b >= hi:
        b = _h16_neighbour(mode, b, False)
    return a, b


def _uniform_candidates(mode, words, lo, hi):
    """What the stored uniform may be: the unfused or the fused float32 evaluation, rounded once to the output format inside it."""
    a, b = _stored_range(mode, lo, hi)
    return [np.clip(half_round(mode, v), a, b) for v in P.uniform(words, lo, hi)]


UNIFORM_RANGES = [(0.0, 1.0), (0.0, 1.0 / 128), (1.0, 2.0), (0.5, 1.5), (-3.0, 5.0), (0.1, 0.7)]


@pytest.mark.parametrize("lo,hi", UNIFORM_RANGES)
def test_rng_uniform_transform(dev, lo, hi):
    ctx, mode = dev
    seed, start = 77, 12
    got = _draw(ctx, COUNT, mode, 0, lo, hi, seed, _state(ctx, start))
    unfused, fused = _uniform_candidates(mode, P.stream_words(seed, start, COUNT), lo, hi)
    ok = (_bits(got) == _bits(unfused)) | (_bits(got) == _bits(fused))
    assert ok.all(), "uniform (%g, %g): %d of %d are neither evaluation, first %r (unfused %r, fused %r)" % (
        lo, hi, (~ok).sum(), COUNT, got[~ok][0], unfused[~ok][0], fused[~ok][0])
    if lo == 0:
        assert unfused is fused or np.array_equal(unfused, fused)          # exactly hi * u
    assert (got >= np.float32(lo)).all() and (got < np.float32(hi)).all()


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (0.0, 1.0 / 128), (1.0, 2.0), (0.5, 1.5)])
def test_rng_uniform_range_at_extreme_words(dev, lo, hi):
    """[lo, hi) in the output type where the stream holds r >> 8 == 0xFFFFFF (the plain float32 expression gives hi for (1, 2) and
    (0.5, 1.5), and 0.0078124995 rounds to 1/128 in bf16) and == 0 (exactly lo)."""
    ctx, mode = dev
    lo32, hi32 = np.float32(lo), np.float32(hi)
    top = _stored_range(mode, lo, hi)[1]
    for quad, lane in P.ALL_ONES_WORDS:
        got = _draw(ctx, 4, mode, 0, lo, hi, P.EXTREME_SEED, _state(ctx, quad))
        print("all-ones word at quad %d lane %d, (%g, %g) %s: %r" % (quad, lane, lo, hi, mode, got[lane]))
        assert got[lane] < hi32, "uniform (%g, %g) in %s returned %r at the all-ones word" % (lo, hi, mode, got[lane])
        assert (got >= lo32).all() and (got < hi32).all()
        assert got[lane] == top or mode == "f32"       # 16-bit: the largest value below hi; f32 with lo = 0: hi * (1 - 2^-24) below it
        if mode == "f32" and lo == 0:
            assert got[lane] == hi32 * np.float32(1 - 2.0 ** -24)
    for quad, lane in P.ZERO_WORDS:
        got = _draw(ctx, 4, mode, 0, lo, hi, P.EXTREME_SEED, _state(ctx, quad))
        assert got[lane] == lo32, (quad, lane, got[lane])
        assert (got >= lo32).all() and (got < hi32).all()


def test_rng_uniform_rejects_what_it_cannot_honour(dev):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    y = Out(ctx, (4,), TDT[mode])
    bad = [(1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)]
    if mode in HALF:
        bad.append((1.0001, 1.0002))            # no 16-bit value in between
    for lo, hi in bad:
        torch.cuda.synchronize()
        assert ctx.lib.rcgan_rng_fill(ctx.h, 4, _code(mode), 0, lo, hi, 1, None, y.ptr) == L.EINVALID_ARG, (lo, hi)
    ctx.sync()
    assert y.intact() and bool(torch.isnan(y.t).all())


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (1.5, 3.0), (-2.0, 0.05)])
def test_rng_normal(dev, mean, std, capsys):
    """Box-Muller against float64 log / sqrt / cos / sin of the float32 u1, u2 and angle (bound: philox_ref.normal_bound)."""
    ctx, mode = dev
    seed, start, count = 555, 7, 4099
    got = _draw(ctx, count, mode, 1, mean, std, seed, _state(ctx, start)).astype(np.float64)
    ref = P.normal(P.stream_quads(seed, start, P.quads_of(count)).reshape(-1), mean, std)[:count]
    bound = P.normal_bound(ref, std)
    assert np.isfinite(got).all()
    if mode == "f32":
        ratio = np.abs(got - ref) / bound
        with capsys.disabled():
            print("\nBox-Muller (%g, %g): worst |got - ref| / bound = %.3f" % (mean, std, ratio.max()))
        assert ratio.max() <= 1.0, "worst ratio %.3f at %d: got %r ref %r" % (ratio.max(), ratio.argmax(), got[ratio.argmax()], ref[ratio.argmax()])
    else:       # one rounding of a float32 value inside the bound
        lo16 = half_round(mode, np.nextafter((ref - bound).astype(np.float32), np.float32(-np.inf)))
        hi16 = half_round(mode, np.nextafter((ref + bound).astype(np.float32), np.float32(np.inf)))
        bad = (got < lo16) | (got > hi16)
        assert not bad.any(), "%d outside, first: got %r ref %r" % (bad.sum(), got[bad][0], ref[bad][0])


def test_rng_normal_at_extreme_words(dev):
    ctx, mode = dev
    mean, std = 0.25, 2.0
    # u1 = 2^-25, the smallest: the largest radius, finite
    quad, lane = [w for w in P.ZERO_WORDS if w[1] == 0][0]
    got = _draw(ctx, 4, mode, 1, mean, std, P.EXTREME_SEED, _state(ctx, quad)).astype(np.float64)
    ref = P.normal(P.stream_quads(P.EXTREME_SEED, quad, 1).reshape(-1), mean, std)
    assert np.isfinite(got).all()
    # (16-bit: one rounding on top, half an ulp <= 2^-8 |x| in bf16 and 2^-11 |x| in fp16)
    slack = P.normal_bound(ref, std) + (np.abs(ref) * (2.0 ** -8 if mode == "bf16" else 2.0 ** -11) if mode in HALF else 0.0)
    assert (np.abs(got[:2] - mean) <= P.RADIUS_MAX * std + slack[:2]).all(), got
    assert (np.abs(got - ref) <= slack).all(), (got, ref)
    assert abs(np.hypot(got[0] - mean, got[1] - mean) - P.RADIUS_MAX * std) <= 2 * slack.max()
    # u1 rounds to 1.0 (r >> 8 == 0xFFFFFF in an even lane): radius 0, both numbers of the pair are exactly the mean
    quad, lane = P.ALL_ONES_EVEN_LANE
    got = _draw(ctx, 4, mode, 1, mean, std, P.EXTREME_SEED, _state(ctx, quad))
    assert got[lane] == np.float32(mean) and got[lane + 1] == np.float32(mean), got
