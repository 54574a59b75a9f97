"""rcgan_diffaugment_gated_fwd / rcgan_diffaugment_sampled_bwd (csrc/augment.hip): the per-sample policy against its restatement
(tests/ada_ref.py, exact), the images against the BITS of rcgan_diffaugment_fwd / _bwd run on the same rows under each sample's
policy -- an exact comparison with the existing entry points, which test_gpu_diffaugment_ops.py holds to the float64 definition --
and, beside that, against the float64 reference directly at that file's bounds (TOL, restated here: fp32 1e-5, one rounding of the
16-bit output format on top).

Draws are diffaugment_ref.draws (every extreme of u, then random rows); the gate rows are built by hand so that all eight gate
combinations occur at p = 0.5, with gates exactly equal to p among those that must NOT be applied (ada_ref.gates).  A shape of n
images is launched n rows at a time until the list is used up.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ada_ref as A
from tests import diffaugment_ref as R
from tests.gpu_util import assert_close, half_round, make_ctx

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 32, 3),       # the production geometry
          (5, 8, 12, 3),        # not square, the smallest windows
          (1, 4, 4, 3),
          (2, 64, 64, 3)]       # 96 KiB of LDS: past the 64 KiB a launch gets by default, the kernel's limit is raised
MODES = ("f32", "bf16", "f16")
TOL = {"f32": 1e-5, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
P_MID = 0.5

_ctx = {}
_data = {}


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
    """(u [m, 8], gate_u [m, 4], x, dy, prefill) as float32, m a multiple of n: computed once per shape, never changed."""
    if shape not in _data:
        n, h, w, c = shape
        u = R.draws(n, 300 + h + w)
        rs = np.random.RandomState(n * 11 + h)
        mk = lambda: rs.uniform(-1.0, 1.0, size=(len(u), h, w, c)).astype(np.float32)
        _data[shape] = (u, A.gates(len(u), P_MID), mk(), half_round("bf16", mk()), mk())
    return _data[shape]


def bits(ctx, t):
    ctx.sync()                     # (the copy below runs on torch's stream, the launches on the context's)
    v = ctx.view(t)
    return v.view(torch.int32 if v.dtype == torch.float32 else torch.int16).cpu()


def P(t):
    return C.c_void_p(t.ptr) if t is not None else None


def set_p(ctx, p_dev, value):
    with torch.cuda.stream(ctx.stream):
        ctx.view(p_dev).fill_(float(value))


class Run:
    """Device buffers of one shape's whole draw list; every entry point over it, n rows per launch."""

    def __init__(self, ctx, shape, x_host, prefill=None):
        from rcgan_amd import _lib as L
        self.ctx, self.shape, self.L = ctx, shape, L
        n, h, w, c = shape
        u, g = data_of(shape)[:2]
        self.m = len(u)
        ctx.arena.reset()
        self.x, self.u, self.g = ctx.upload(x_host), ctx.upload(u, dtype=L.F32), ctx.upload(g, dtype=L.F32)
        self.p = ctx.upload(np.zeros(1, np.float32), dtype=L.F32)
        self.prefill = prefill

    def out(self):
        n, h, w, c = self.shape
        return self.ctx.upload(self.prefill) if self.prefill is not None else self.ctx.empty((self.m, h, w, c))

    def gated_fwd(self, policy, p, pool=True):
        ctx = self.ctx
        n, h, w, c = self.shape
        y, yp = self.out(), (ctx.empty((self.m, h // 2, w // 2, c)) if pool else None)
        sp = ctx.upload(np.full(self.m, -7, np.int32))
        set_p(ctx, self.p, p)
        for lo in range(0, self.m, n):
            ctx.check(ctx.lib.rcgan_diffaugment_gated_fwd(
                ctx.h, n, h, w, self.x.dtype, policy, P(self.x.rows(lo, lo + n)), P(self.u.rows(lo, lo + n)), P(self.g.rows(lo, lo + n)),
                P(self.p), P(y.rows(lo, lo + n)), P(yp.rows(lo, lo + n)) if pool else None, P(sp.rows(lo, lo + n))))
        return y, yp, sp

    def plain(self, policy, bwd=False, pool=True):
        """rcgan_diffaugment_fwd / _bwd over every row under ONE policy."""
        ctx = self.ctx
        n, h, w, c = self.shape
        y = self.out()
        yp = ctx.empty((self.m, h // 2, w // 2, c)) if (pool and not bwd) else None
        for lo in range(0, self.m, n):
            a = (ctx.h, n, h, w, self.x.dtype, policy, P(self.x.rows(lo, lo + n)), P(self.u.rows(lo, lo + n)), P(y.rows(lo, lo + n)))
            if bwd:
                ctx.check(ctx.lib.rcgan_diffaugment_bwd(*a, 1 if self.prefill is not None else 0))
            else:
                ctx.check(ctx.lib.rcgan_diffaugment_fwd(*a, P(yp.rows(lo, lo + n)) if yp is not None else None))
        return y, yp

    def sampled_bwd(self, sp):
        ctx = self.ctx
        n, h, w, c = self.shape
        dx = self.out()
        for lo in range(0, self.m, n):
            ctx.check(ctx.lib.rcgan_diffaugment_sampled_bwd(
                ctx.h, n, h, w, self.x.dtype, P(self.x.rows(lo, lo + n)), P(self.u.rows(lo, lo + n)), P(sp.rows(lo, lo + n)),
                P(dx.rows(lo, lo + n)), 1 if self.prefill is not None else 0))
        return dx

    def per_sample(self, pol, bwd=False):
        """The bits the existing entry point gives every row under that row's own policy: (output, pooled output) int tensors."""
        out = pooled = None
        for q in sorted(set(pol.tolist())):
            y, yp = self.plain(int(q), bwd=bwd)
            yb = bits(self.ctx, y)
            out = yb.clone() if out is None else out
            rows = torch.from_numpy(pol == q)
            out[rows] = yb[rows]
            if yp is not None:
                pb = bits(self.ctx, yp)
                pooled = pb.clone() if pooled is None else pooled
                pooled[rows] = pb[rows]
        return out, pooled


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_forward_policy_images_and_pooled_output(mode, shape):
    ctx = ctx_of(mode)
    u, g, x, _, _ = data_of(shape)
    r = Run(ctx, shape, x)
    for policy in (7, 5):
        want_pol = A.sample_policy(g, P_MID, policy)
        if policy == 7:
            assert sorted(set(want_pol.tolist())) == list(range(8)), "every gate combination occurs"
        y, yp, sp = r.gated_fwd(policy, P_MID)
        got_pol = ctx.download(sp)
        assert got_pol.dtype == np.int32 and np.array_equal(got_pol, want_pol), (policy, got_pol, want_pol)
        want, want_pool = r.per_sample(want_pol)
        assert torch.equal(bits(ctx, y), want), "y, policy %d" % policy
        assert torch.equal(bits(ctx, yp), want_pool), "y_pool, policy %d" % policy
        # without the pooled output: the same y
        y2, _, sp2 = r.gated_fwd(policy, P_MID, pool=False)
        assert torch.equal(bits(ctx, y2), want) and np.array_equal(ctx.download(sp2), want_pol)
    # the float64 definition, at the bounds of the ungated entry points
    xr = torch.from_numpy(half_round(mode, x).astype(np.float64))
    yref = A.diffaugment(xr, u, g, P_MID, 7).numpy()
    y, _, _ = r.gated_fwd(7, P_MID)
    got = ctx.download(y)
    print("gated fwd %s %s: max err %.3e of max|ref| (bound %.3e)" % (mode, shape, np.abs(got - yref).max() / np.abs(yref).max(), TOL[mode]))
    assert_close(got, yref, TOL[mode], "y against float64")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_p_zero_copies_and_p_one_is_the_ungated_launch(mode, shape):
    ctx = ctx_of(mode)
    u, g, x, _, _ = data_of(shape)
    g0 = g.copy()
    g0[0, :] = 0.0                     # not even a zero gate passes p = 0 ...
    g0[1, :] = R.U_MAX                 # ... and the largest gate a draw can give passes p = 1
    r = Run(ctx, shape, x)
    r.g = ctx.upload(g0, dtype=r.L.F32)
    y, yp, sp = r.gated_fwd(7, 0.0)
    assert torch.equal(bits(ctx, y), bits(ctx, r.x)), "p = 0: a bit copy of x"
    assert (ctx.download(sp) == 0).all()
    want, want_pool = r.plain(0)
    assert torch.equal(bits(ctx, yp), bits(ctx, want_pool))
    for policy in (7, 6):
        y, yp, sp = r.gated_fwd(policy, 1.0)
        want, want_pool = r.plain(policy)
        assert torch.equal(bits(ctx, y), bits(ctx, want)) and torch.equal(bits(ctx, yp), bits(ctx, want_pool)), policy
        assert (ctx.download(sp) == policy).all()
    # a NaN p applies nothing
    y, _, sp = r.gated_fwd(7, float("nan"))
    assert torch.equal(bits(ctx, y), bits(ctx, r.x)) and (ctx.download(sp) == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_adjoint_under_the_recorded_policies(mode, shape):
    ctx = ctx_of(mode)
    u, g, _, dy, pre = data_of(shape)
    dy = half_round(mode if mode == "f16" else "bf16", dy)
    want_pol = A.sample_policy(g, P_MID, 7)
    for prefill in (None, half_round(mode, pre)):
        r = Run(ctx, shape, dy, prefill=prefill)
        sp = ctx.upload(want_pol)
        dx = r.sampled_bwd(sp)
        want, _ = r.per_sample(want_pol, bwd=True)
        assert torch.equal(bits(ctx, dx), want), "dx, accumulate %d" % (prefill is not None)
    # bits above the three policy bits are not looked at
    r = Run(ctx, shape, dy)
    dx = r.sampled_bwd(ctx.upload(want_pol | np.int32(8)))
    assert torch.equal(bits(ctx, dx), r.per_sample(want_pol, bwd=True)[0])
    # the float64 adjoint (autograd through the restatement)
    xr = torch.zeros((len(u),) + shape[1:], dtype=torch.float64, requires_grad=True)
    (dxref,) = torch.autograd.grad((A.diffaugment(xr, u, g, P_MID, 7) * torch.from_numpy(dy.astype(np.float64))).sum(), xr)
    assert_close(ctx.download(dx), dxref.numpy(), TOL[mode], "dx against float64")


def test_p_is_read_on_the_device_when_the_launch_runs():
    ctx = ctx_of("f32")
    shape = SHAPES[1]
    n, h, w, c = shape
    u, g, x, _, _ = data_of(shape)
    r = Run(ctx, shape, x)
    y, sp_a, sp_b = r.out(), ctx.upload(np.full(n, -7, np.int32)), ctx.upload(np.full(n, -7, np.int32))
    args = lambda sp: (ctx.h, n, h, w, r.x.dtype, 7, P(r.x.rows(0, n)), P(r.u.rows(0, n)), P(r.g.rows(0, n)), P(r.p), P(y.rows(0, n)), None, P(sp))
    set_p(ctx, r.p, 0.0)
    ctx.check(ctx.lib.rcgan_diffaugment_gated_fwd(*args(sp_a)))
    set_p(ctx, r.p, P_MID)             # the same host arguments: only the device value moved
    ctx.check(ctx.lib.rcgan_diffaugment_gated_fwd(*args(sp_b)))
    a, b = ctx.download(sp_a), ctx.download(sp_b)
    assert (a == 0).all() and np.array_equal(b, A.sample_policy(g[:n], P_MID, 7)) and not np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tape_op_records_the_sampled_adjoint(mode):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx = ctx_of(mode)
    shape = SHAPES[0]
    n, h, w, c = shape
    u_all, g_all, x_all, dy_all, _ = data_of(shape)
    lo = 30
    u_host, g_host, x_host = u_all[lo:lo + n], A.gate_rows(P_MID)[[3, 5, 6]], x_all[lo:lo + n]
    dy = half_round(mode if mode == "f16" else "bf16", dy_all[lo:lo + n])
    xr = torch.from_numpy(half_round(mode, x_host).astype(np.float64)).requires_grad_(True)
    yref = A.diffaugment(xr, u_host, g_host, P_MID, 7)
    (dxref,) = torch.autograd.grad((yref * torch.from_numpy(dy.astype(np.float64))).sum(), xr)
    ctx.arena.reset()
    ctx.tape = []
    x, u, g = ctx.upload(x_host), ctx.upload(u_host, dtype=L.F32), ctx.upload(g_host, dtype=L.F32)
    p = torch.tensor([P_MID], dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    y, yp = O.diffaugment(ctx, x, u, 7, pool=True, gate=g, p=p)
    assert not y.req and ctx.tape == [] and yp.shape == (n, h // 2, w // 2, 3)
    assert_close(ctx.download(y), yref.detach().numpy(), TOL[mode], "y")
    xf = x.reshape((n, h * w * c))
    xf.req = True
    yf = O.diffaugment(ctx, xf, u, 7, gate=g, p=p)
    assert yf.req and len(ctx.tape) == 1
    # p moves between the forward and its backward: the adjoint follows what the forward recorded
    ctx.sync()
    p.fill_(0.0)
    torch.cuda.synchronize()
    yf.grad = ctx.upload(dy.reshape(n, -1))
    ctx.backward()
    assert_close(ctx.download(xf.grad).reshape(shape), dxref.numpy(), TOL[mode], "dx from the tape")
    with pytest.raises(ValueError, match="gate and p come together"):
        O.diffaugment(ctx, x, u, 7, gate=g)
    with pytest.raises(ValueError, match=r"fp32 \[3, 4\]"):
        O.diffaugment(ctx, x, u, 7, gate=u, p=p)


def test_refused_calls_launch_nothing():
    from rcgan_amd import _lib as L
    ctx = ctx_of("f32")
    ctx.arena.reset()
    n, h, w = 2, 8, 8
    sentinel = np.full((n, h, w, 3), 7.0, np.float32)
    x, y, yp = ctx.upload(sentinel), ctx.upload(sentinel), ctx.upload(sentinel[:, :4, :4])
    u = ctx.upload(np.full((n, 8), 0.5, np.float32), dtype=L.F32)
    g = ctx.upload(np.zeros((n + 1, 4), np.float32), dtype=L.F32)
    p = ctx.upload(np.ones(2, np.float32), dtype=L.F32)
    sp = ctx.upload(np.full(n + 1, -7, np.int32))
    good = dict(gate_u=g.ptr, p_dev=p.ptr, sample_policy=sp.ptr)

    def fwd(**kw):
        a = dict(good)
        a.update(kw)
        return ctx.lib.rcgan_diffaugment_gated_fwd(ctx.h, kw.get("n", n), kw.get("h", h), w, L.F32, kw.get("policy", 7), P(x), P(u),
                                                   a["gate_u"], a["p_dev"], P(y), P(yp), a["sample_policy"])
    for name in good:
        for bad in (None, good[name] + 2, good[name] + 1):
            assert fwd(**{name: bad}) == L.EINVALID_ARG, (name, bad)
            assert ctx.lib.rcgan_last_error(ctx.h)
    for bad in (dict(n=0), dict(policy=8), dict(h=6)):
        assert fwd(**bad) == L.EINVALID_ARG, bad
    for bad in (None, sp.ptr + 2):
        assert ctx.lib.rcgan_diffaugment_sampled_bwd(ctx.h, n, h, w, L.F32, P(x), P(u), bad, P(y), 0) == L.EINVALID_ARG
    assert ctx.lib.rcgan_diffaugment_sampled_bwd(ctx.h, n, 6, w, L.F32, P(x), P(u), P(sp), P(y), 0) == L.EINVALID_ARG
    # the controller
    st_host = np.array([0.25, 1, 2, 3, 0.5, 4, 0, 0], np.float32)
    st = ctx.upload(st_host, dtype=L.F32)
    lg = ctx.upload(np.ones((4, 2), np.float32), dtype=L.F32)
    lab = ctx.upload(np.zeros(4, np.int32))

    def upd(n=4, ld=2, logits=lg.ptr, labels=lab.ptr, state=st.ptr, images=100.0, interval=1):
        return ctx.lib.rcgan_ada_update(ctx.h, n, logits, ld, labels, state, 0.6, images, interval)
    for bad in (dict(interval=0), dict(interval=-1), dict(images=0.0), dict(images=-1.0), dict(images=float("nan")), dict(n=0), dict(ld=0),
                dict(logits=None), dict(state=None), dict(state=st.ptr + 2), dict(logits=lg.ptr + 1), dict(labels=lab.ptr + 2)):
        assert upd(**bad) == L.EINVALID_ARG, bad
        assert ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(ctx.download(y), sentinel) and np.array_equal(ctx.download(yp), sentinel[:, :4, :4]), "a refused call wrote"
    assert (ctx.download(sp) == -7).all() and np.array_equal(ctx.download(st), st_host)
    # ... and the same arguments, put right, run
    assert fwd() == 0 and upd() == 0
    ctx.sync()
    assert (ctx.download(sp)[:n] == 7).all() and ctx.download(sp)[n] == -7
    assert np.array_equal(ctx.download(st), A.update(st_host, np.ones((4, 2), np.float32), np.zeros(4, np.int32), 0.6, 100.0, 1))
