"""rcgan_diffaugment_fwd / _bwd (csrc/augment.hip) against the float64 restatement of the definition (tests/diffaugment_ref.py) and
its autograd adjoint.

Draws are explicit: the hand-built rows at every extreme (u = 0 and u = 0.99999994 in each slot -- s = 0 and k = 0.5 among them --
and every combination of the translation extremes with the cutout extremes) followed by random rows.  A shape of n images is
launched with n rows at a time until the list is used up, so the one-image shape sees every extreme too.

Bounds, all by gpu_util.assert_close (max error relative to the reference's largest magnitude): fp32 1e-5, the bound of the fp32 loss
tests -- the op is a dozen flops and two short means; 16-bit output 2^-8 (bf16) / 2^-11 (fp16): one rounding of the output format
plus the fp32 error.  dy is 16-bit rounded before either side sees it, in every mode.

"Exactly 0.0 outside the support" is asserted for the policies without COLOR: the contrast and saturation adjoints spread the mean
of the gradient over every pixel of the sample, cut out or not, so with COLOR the gradient there is not zero by definition (the
reference agrees: tests/test_diffaugment_cpu.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import diffaugment_ref as R
from tests.gpu_util import assert_close, half_round, make_ctx

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 32, 3),       # the production geometry
          (5, 8, 12, 3),        # not square, the smallest windows: shifts 1 and 2, cutout 4 x 6
          (1, 4, 4, 3),
          (128, 32, 32, 3),     # the generator step's row count
          (2, 64, 64, 3)]       # 96 KiB of LDS: past the 64 KiB a launch gets by default, the kernel's limit is raised
MODES = ("f32", "bf16", "f16")
TOL = {"f32": 1e-5, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}

_ctx = {}
_data = {}
_ref = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def ctx_of(mode):
    if mode not in _ctx:
        _ctx[mode] = make_ctx(mode, arena=256 << 20)
    return _ctx[mode]


def data_of(shape):
    """(u [m, 8], x [m, h, w, 3], dy, prefill) as float32, m a multiple of n: computed once per shape."""
    if shape not in _data:
        n, h, w, c = shape
        u = R.draws(n, 100 + h + w)
        rs = np.random.RandomState(n * 7 + h)
        mk = lambda: rs.uniform(-1.0, 1.0, size=(len(u), h, w, c)).astype(np.float32)
        _data[shape] = (u, mk(), half_round("bf16", mk()), mk())
    return _data[shape]


def reference(shape, mode, policy):
    """float64: (y, dx) on the inputs as the device sees them in ``mode`` (x rounded to the storage format, dy to 16 bits)."""
    key = (shape, mode, policy)
    if key not in _ref:
        u, x, dy, _ = data_of(shape)
        xr = torch.from_numpy(half_round(mode, x).astype(np.float64)).requires_grad_(True)
        y = R.diffaugment(xr, u, policy)
        (dx,) = torch.autograd.grad((y * torch.from_numpy(half_round(mode if mode == "f16" else "bf16", dy).astype(np.float64))).sum(), xr)
        _ref[key] = (y.detach().numpy(), dx.numpy())
    return _ref[key]


def dy_of(shape, mode):
    """dy, 16-bit rounded before both sides see it (bf16; the fp16 build stores fp16)."""
    return half_round(mode if mode == "f16" else "bf16", data_of(shape)[2])


def bits(ctx, t):
    v = ctx.view(t)
    return v.view(torch.int32 if v.dtype == torch.float32 else torch.int16).cpu()


def run(ctx, shape, policy, x_host, u_host, pool=False, bwd=False, prefill=None):
    """The entry point over every row of the draw list, n rows per launch -> (output, pooled output) device tensors."""
    from rcgan_amd import _lib as L
    n, h, w, c = shape
    m = len(u_host)
    ctx.arena.reset()
    x = ctx.upload(x_host)
    u = ctx.upload(u_host, dtype=L.F32)
    out = ctx.upload(prefill) if prefill is not None else ctx.empty((m, h, w, c))
    yp = ctx.empty((m, h // 2, w // 2, c)) if pool else None
    for lo in range(0, m, n):
        xs, us, os_ = x.rows(lo, lo + n), u.rows(lo, lo + n), out.rows(lo, lo + n)
        if bwd:
            rc = ctx.lib.rcgan_diffaugment_bwd(ctx.h, n, h, w, x.dtype, policy, C.c_void_p(xs.ptr), C.c_void_p(us.ptr), C.c_void_p(os_.ptr),
                                               1 if prefill is not None else 0)
        else:
            ps = C.c_void_p(yp.rows(lo, lo + n).ptr) if pool else None
            rc = ctx.lib.rcgan_diffaugment_fwd(ctx.h, n, h, w, x.dtype, policy, C.c_void_p(xs.ptr), C.c_void_p(us.ptr), C.c_void_p(os_.ptr), ps)
        ctx.check(rc)
    return out, yp


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_forward_and_pooled_output(mode, shape):
    from rcgan_amd import _lib as L
    ctx = ctx_of(mode)
    u, x, _, _ = data_of(shape)
    n, h, w, c = shape
    for policy in R.POLICIES:
        yref, _ = reference(shape, mode, policy)
        y, yp = run(ctx, shape, policy, x, u, pool=True)
        got = ctx.download(y)
        err = np.abs(got - yref).max() / np.abs(yref).max()
        print("fwd %s %s policy %d: max err %.3e of max|ref| (bound %.3e)" % (mode, shape, policy, err, TOL[mode]))
        assert_close(got, yref, TOL[mode], "y policy %d" % policy)
        # the pooled output: the bits of rcgan_meanpool2_fwd on the y the launch wrote
        want = ctx.empty(yp.shape)
        ctx.check(ctx.lib.rcgan_meanpool2_fwd(ctx.h, len(u), h, w, c, y.dtype, C.c_void_p(y.ptr), C.c_void_p(want.ptr)))
        assert torch.equal(bits(ctx, yp), bits(ctx, want)), "pooled output, policy %d" % policy
        # ... and a launch without the pooled output writes the same y
        y2, _ = run(ctx, shape, policy, x, u, pool=False)
        assert np.array_equal(ctx.download(y2), got), "y without pool, policy %d" % policy
    # policy 0: a copy
    y0, _ = run(ctx, shape, 0, x, u)
    assert np.array_equal(ctx.download(y0), half_round(mode, x))
    assert ctx.act_dtype == {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}[mode]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_adjoint(mode, shape):
    ctx = ctx_of(mode)
    u, x, _, pre = data_of(shape)
    n, h, w, c = shape
    dy = dy_of(shape, mode)
    pre = half_round(mode, pre)
    for policy in R.POLICIES:
        _, dxref = reference(shape, mode, policy)
        dx, _ = run(ctx, shape, policy, dy, u, bwd=True)
        got = ctx.download(dx)
        err = np.abs(got - dxref).max() / np.abs(dxref).max()
        print("bwd %s %s policy %d: max err %.3e of max|ref| (bound %.3e)" % (mode, shape, policy, err, TOL[mode]))
        assert_close(got, dxref, TOL[mode], "dx policy %d" % policy)
        # accumulate = 1 adds to what dx holds
        acc, _ = run(ctx, shape, policy, dy, u, bwd=True, prefill=pre)
        assert_close(ctx.download(acc), dxref + pre, TOL[mode], "dx accumulated, policy %d" % policy)
        if not policy & R.COLOR:
            sup = R.support(u, h, w, policy)
            assert (got[~sup] == 0.0).all(), "gradient outside the support, policy %d" % policy
            assert (sup.sum(axis=(1, 2)) < h * w).any()
        if mode == "f32":
            # <A(x) - A(0), dy> = <x, A^T dy> (the map is affine), to 1e-5 relative
            ax = ctx.download(run(ctx, shape, policy, x, u)[0]).astype(np.float64)
            a0 = ctx.download(run(ctx, shape, policy, np.zeros_like(x), u)[0]).astype(np.float64)
            lhs, rhs = float(((ax - a0) * dy).sum()), float((x.astype(np.float64) * got).sum())
            print("adjoint identity %s policy %d: %.9e vs %.9e" % (shape, policy, lhs, rhs))
            assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (policy, lhs, rhs)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tape_op_records_the_adjoint_only_for_a_tracked_input(mode):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx = ctx_of(mode)
    shape = SHAPES[0]
    n, h, w, c = shape
    u_all, x_all, _, _ = data_of(shape)
    u_host, x_host, policy = u_all[30:30 + n], x_all[30:30 + n], 7
    dy = dy_of(shape, mode)[30:30 + n]
    xr = torch.from_numpy(half_round(mode, x_host).astype(np.float64)).requires_grad_(True)
    yref = R.diffaugment(xr, u_host, policy)
    (dxref,) = torch.autograd.grad((yref * torch.from_numpy(dy.astype(np.float64))).sum(), xr)
    ctx.arena.reset()
    ctx.tape = []
    x, u = ctx.upload(x_host), ctx.upload(u_host, dtype=L.F32)
    # not tracked: nothing on the tape, the pooled tensor comes back beside y
    y, yp = O.diffaugment(ctx, x, u, policy, pool=True)
    assert not y.req and ctx.tape == [] and yp.shape == (n, h // 2, w // 2, 3) and y.shape == x.shape
    assert_close(ctx.download(y), yref.detach().numpy(), TOL[mode], "y")
    # tracked, as flattened rows (the generator's output): the adjoint runs from the tape
    xf = x.reshape((n, h * w * c))
    xf.req = True
    yf = O.diffaugment(ctx, xf, u, policy)
    assert yf.req and len(ctx.tape) == 1 and yf.shape == xf.shape
    assert np.array_equal(ctx.download(yf).reshape(shape), ctx.download(y))
    yf.grad = ctx.upload(dy.reshape(n, -1))
    ctx.backward()
    assert_close(ctx.download(xf.grad).reshape(shape), dxref.numpy(), TOL[mode], "dx from the tape")
    # a second contribution accumulates
    yf2 = O.diffaugment(ctx, xf, u, policy)
    yf2.grad = ctx.upload(dy.reshape(n, -1))
    ctx.backward()
    assert_close(ctx.download(xf.grad).reshape(shape), 2 * dxref.numpy(), TOL[mode], "dx accumulated on the tape")


def test_bad_shapes_are_refused_without_a_launch():
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx = ctx_of("f32")
    ctx.arena.reset()
    ctx.tape = []
    sentinel = np.full((2, 6, 8, 3), 7.0, np.float32)
    x, y = ctx.upload(sentinel), ctx.upload(sentinel)
    u = ctx.upload(np.full((2, 8), 0.5, np.float32), dtype=L.F32)
    rc = ctx.lib.rcgan_diffaugment_fwd(ctx.h, 2, 6, 8, L.F32, 7, C.c_void_p(x.ptr), C.c_void_p(u.ptr), C.c_void_p(y.ptr), None)
    assert rc == L.EINVALID_ARG and b"multiples of 4" in ctx.lib.rcgan_last_error(ctx.h)
    rc = ctx.lib.rcgan_diffaugment_bwd(ctx.h, 2, 6, 8, L.F32, 7, C.c_void_p(x.ptr), C.c_void_p(u.ptr), C.c_void_p(y.ptr), 0)
    assert rc == L.EINVALID_ARG and b"multiples of 4" in ctx.lib.rcgan_last_error(ctx.h)
    with pytest.raises(L.RcganError, match="multiples of 4"):
        O.diffaugment(ctx, x, u, 7)
    for bad in (dict(n=0), dict(policy=8), dict(h=128, w=128)):
        a = dict(n=2, h=8, w=8, policy=7)
        a.update(bad)
        rc = ctx.lib.rcgan_diffaugment_fwd(ctx.h, a["n"], a["h"], a["w"], L.F32, a["policy"], C.c_void_p(x.ptr), C.c_void_p(u.ptr), C.c_void_p(y.ptr), None)
        assert rc == L.EINVALID_ARG and ctx.lib.rcgan_last_error(ctx.h), bad
    # c != 3: refused by the op (the entry points take 3-channel images only)
    x4 = ctx.upload(np.zeros((2, 8, 8, 4), np.float32))
    with pytest.raises(ValueError, match="3-channel"):
        O.diffaugment(ctx, x4, u, 7)
    with pytest.raises(ValueError, match=r"fp32 \[2, 8\]"):
        O.diffaugment(ctx, ctx.upload(np.zeros((2, 8, 8, 3), np.float32)), ctx.upload(np.zeros((3, 8), np.float32), dtype=L.F32), 7)
    assert np.array_equal(ctx.download(y), sentinel), "a refused call wrote its output"
