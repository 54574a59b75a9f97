"""The kernels behind classifier training (csrc/classifier.hip) against float64 / exact restatements: sparse softmax cross-entropy,
the option-A shortcut and its adjoint, the momentum optimiser, the input pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import classifier_ref as R
from tests.gpu_util import FakeParam, assert_close, make_ctx

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32")
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ softmax cross-entropy
def _xent_case(rows, cols, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-80, 80, size=(rows, cols)).astype(np.float32)
    lab = rs.randint(cols, size=rows)
    for r in range(0, rows, 3):                      # deliberate ties of the row maximum: the lower index wins, as numpy.argmax
        a, b = sorted(rs.choice(cols, 2, replace=False))
        x[r, a] = x[r, b] = x[r].max() + 1.0
        lab[r] = a if (r // 3) % 2 == 0 else b       # ... labelled right in half of them, on the losing twin in the others
    for r in range(1, rows, 3):                      # and rows the arg-max gets right without a tie
        lab[r] = int(np.argmax(x[r]))
    return x, lab.astype(np.int32)


def _xent_ref(x, lab, weight):
    x = x.astype(np.float64)
    m = x.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(1))
    p = np.exp(x - lse[:, None])
    onehot = np.zeros_like(p)
    onehot[np.arange(len(lab)), lab] = 1
    return weight * float((lse - x[np.arange(len(lab)), lab]).mean()), weight * (p - onehot) / len(lab), int((np.argmax(x, 1) == lab).sum())


@pytest.mark.parametrize("rows,cols", [(1, 2), (7, 10), (128, 100), (1000, 100), (33, 1024)])
def test_softmax_xent_against_float64(ctx, rows, cols):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    x, lab = _xent_case(rows, cols, rows * 7 + cols)
    weight = 0.75
    L_ref, d_ref, n_ref = _xent_ref(x, lab, weight)
    ctx.new_step()
    ctx.recording = True
    lg = FakeParam(ctx, x)
    labels = ctx.upload(lab)
    loss, ncor = ctx.persistent((1,), L.F32, fill=0.0), ctx.persistent((1,), L.F32, fill=0.0)
    O.softmax_xent(ctx, lg.t, labels, weight, loss, ncor)
    got_L, got_n, got_d = float(ctx.download(loss)[0]), float(ctx.download(ncor)[0]), lg.grad(ctx)
    print("xent %dx%d: loss %.7g (float64 %.7g, diff %.2e), n_correct %d (%d), dlogits max err %.2e of %.2e"
          % (rows, cols, got_L, L_ref, abs(got_L - L_ref), got_n, n_ref, np.abs(got_d - d_ref).max(), np.abs(d_ref).max()))
    assert abs(got_L - L_ref) <= 2e-5 * max(1.0, abs(L_ref)), (got_L, L_ref)
    assert got_n == n_ref
    assert_close(got_d, d_ref, 2e-5, "dlogits")
    # the accumulators ADD; evaluation (recording off) writes no gradient and takes no counter; the same bits run to run
    ctx.recording = False
    before = lg.grad(ctx).copy()
    O.softmax_xent(ctx, lg.t, labels, weight, loss)
    ctx.recording = True
    assert _bits(ctx.download(loss))[0] == _bits(np.float32(np.float32(got_L) + np.float32(got_L)))[0]
    assert float(ctx.download(ncor)[0]) == n_ref and (_bits(lg.grad(ctx)) == _bits(before)).all()
    # the gradient (not the loss) follows rcgan_set_grad_scale, as the other loss kernels' do
    loss2 = ctx.persistent((1,), L.F32, fill=0.0)
    ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 8.0, None))
    try:
        O.softmax_xent(ctx, lg.t, labels, weight, loss2)
    finally:
        ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1.0, None))
    assert _bits(ctx.download(loss2))[0] == _bits(np.float32(got_L))[0]
    assert_close(lg.grad(ctx), 8.0 * d_ref, 2e-5, "scaled dlogits")


def test_softmax_xent_rejects_bad_shapes(ctx):
    from rcgan_amd import _lib as L
    x = ctx.persistent((4, 1025), L.F32, fill=0.0)
    lab = ctx.persistent((4,), "i32", fill=0)
    loss = ctx.persistent((1,), L.F32, fill=0.0)
    for cols in (1, 1025):
        rc = ctx.lib.rcgan_softmax_xent_fwd_bwd(ctx.h, 4, cols, C.c_void_p(x.ptr), C.c_void_p(lab.ptr), 1.0, C.c_void_p(loss.ptr), None, None,
                                                C.c_void_p(ctx.ws_ptr), ctx.ws_bytes)
        assert rc == L.EUNSUPPORTED_SHAPE, (cols, rc)


# ------------------------------------------------------------------------------------------------ option-A shortcut
SHAPES = [(3, 32, 32, 16), (2, 16, 16, 32), (1, 2, 2, 2)]


def _shortcut_ref(x):
    n, h, w, c = x.shape
    x = x.astype(np.float64)
    y = np.zeros((n, h // 2, w // 2, 2 * c))
    y[..., c // 2:c // 2 + c] = x.reshape(n, h // 2, 2, w // 2, 2, c).mean(axis=(2, 4))
    return y


def _shortcut_adj_ref(dy, c):
    mid = dy.astype(np.float64)[..., c // 2:c // 2 + c]
    return 0.25 * mid.repeat(2, axis=1).repeat(2, axis=2)


@pytest.mark.parametrize("shape", SHAPES)
def test_shortcut_a_forward_is_meanpool_then_pad_bit_for_bit(ctx, shape):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    n, h, w, c = shape
    x = (np.random.RandomState(c).randn(*shape) * 3).astype(np.float32)
    ctx.new_step()
    ctx.recording = False
    xd = ctx.upload(x, L.F32)
    got = ctx.download(O.shortcut_a(ctx, xd))
    pooled = O.meanpool2(ctx, xd)
    two = ctx.empty((n, h // 2, w // 2, 2 * c), L.F32)
    ctx.check(ctx.lib.rcgan_pad_channels(ctx.h, n * (h // 2) * (w // 2), c, c // 2, c // 2, L.F32, C.c_void_p(pooled.ptr), C.c_void_p(two.ptr)))
    ctx.recording = True
    assert got.shape == (n, h // 2, w // 2, 2 * c)
    assert (_bits(got) == _bits(ctx.download(two))).all()
    assert_close(got, _shortcut_ref(x), 2e-5, "shortcut_a forward")


@pytest.mark.parametrize("shape", SHAPES)
def test_shortcut_a_backward(ctx, shape):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    n, h, w, c = shape
    rs = np.random.RandomState(h + c)
    x = rs.randn(*shape).astype(np.float32)
    dy = rs.randn(n, h // 2, w // 2, 2 * c).astype(np.float32)
    ref = _shortcut_adj_ref(dy, c)
    # first consumer: the adjoint is written
    ctx.new_step()
    ctx.recording = True
    xd = ctx.upload(x, L.F32)
    xd.req = True
    y = O.shortcut_a(ctx, xd)
    y.grad = ctx.upload(dy, L.F32)
    ctx.backward()
    ax, aty = ctx.download(y).astype(np.float64), ctx.download(xd.grad).astype(np.float64)
    assert_close(aty, ref, 2e-5, "shortcut_a backward")
    # <A x, y> = <x, A^T y> in float64 on the downloaded tensors: A^T y is exact (a power of two times dy), every element of A x carries
    # at most three fp32 roundings
    lhs, rhs = float((ax * dy.astype(np.float64)).sum()), float((x.astype(np.float64) * aty).sum())
    assert abs(lhs - rhs) <= 4 * EPS32 * float(np.abs(ax * dy).sum()) + 1e-300, (lhs, rhs)
    # a gradient that is already there is added to
    g0 = rs.randn(*shape).astype(np.float32)
    ctx.new_step()
    xp = FakeParam(ctx, x)
    with torch.cuda.stream(ctx.stream):
        ctx.view(xp.t.grad).copy_(torch.from_numpy(g0))
    y = O.shortcut_a(ctx, xp.t)
    y.grad = ctx.upload(dy, L.F32)
    ctx.backward()
    assert_close(xp.grad(ctx), g0.astype(np.float64) + ref, 2e-5, "shortcut_a backward, accumulate")


# ------------------------------------------------------------------------------------------------ momentum optimiser
@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("decay", ["none", "head", "all"])
def test_sgd_momentum_against_float64(ctx, nesterov, decay):
    count = 64 * 16 + 37                                   # not a multiple of 64 (nor of 4: the scalar tail runs)
    decay_count = {"none": 0, "head": 100, "all": count}[decay]
    rs = np.random.RandomState(3 + nesterov)
    w0 = rs.randn(count).astype(np.float32)
    a0 = (0.1 * rs.randn(count)).astype(np.float32)
    grads = [rs.randn(count).astype(np.float32) for _ in range(3)]
    lrs = [0.1, 0.1, 0.01]
    f32 = lambda v: float(np.float32(v))                    # the hyper-parameters as the kernel receives them
    mom, wd, gs = f32(0.9), f32(1e-4), f32(0.5)
    dev = ctx.device
    with torch.cuda.stream(ctx.stream):
        w, a = torch.from_numpy(w0).to(dev), torch.from_numpy(a0).to(dev)
        hyper = torch.zeros(1, dtype=torch.float32, device=dev)
    wr, ar = w0.astype(np.float64), a0.astype(np.float64)
    bound_w, bound_a = np.zeros(count), np.zeros(count)
    dmask = (np.arange(count) < decay_count).astype(np.float64)
    for g32, lr in zip(grads, lrs):
        with torch.cuda.stream(ctx.stream):
            g = torch.from_numpy(g32).to(dev)
            hyper.fill_(lr)
        ctx.check(ctx.lib.rcgan_sgd_momentum(ctx.h, count, decay_count, w.data_ptr(), g.data_ptr(), a.data_ptr(), hyper.data_ptr(),
                                             0.9, 1e-4, nesterov, 0.5))
        ctx.sync()
        lr = f32(lr)
        # the derived bound: at most five fp32 operations per element and result, each rounding an intermediate no larger than S
        G = np.abs(gs * g32.astype(np.float64)) + np.abs(wd * wr) * dmask
        S_a = np.abs(ar) + G
        S_w = np.abs(wr) + lr * (G + S_a)
        bound_a += 5 * EPS32 * S_a
        bound_w += 5 * EPS32 * S_w
        gp = gs * g32.astype(np.float64) + wd * wr * dmask
        ar = mom * ar + gp
        wr = wr - lr * (gp + mom * ar) if nesterov else wr - lr * ar
    with torch.cuda.stream(ctx.stream):
        got_w, got_a = w.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64)
    ctx.sync()
    ew, ea = np.abs(got_w - wr), np.abs(got_a - ar)
    print("sgd_momentum nesterov=%d decay=%s: worst err / bound: w %.3f, accum %.3f" % (nesterov, decay, (ew / bound_w).max(), (ea / bound_a).max()))
    assert (ea <= bound_a).all(), (ea / bound_a).max()
    assert (ew <= bound_w).all(), (ew / bound_w).max()
    assert np.abs(got_w - w0).max() > 1e-3                 # it moved


# ------------------------------------------------------------------------------------------------ input pipeline
def test_augment_cifar_is_exact(ctx):
    from rcgan_amd import _lib as L
    rs = np.random.RandomState(8)
    N = 40
    images = rs.randint(0, 256, size=(N, 3072)).astype(np.uint8)
    labels_all = rs.randint(100, size=N).astype(np.int32)
    sf = np.array([(dy, dx, fl) for fl in (0, 1) for dy in range(-4, 5) for dx in range(-4, 5)], np.int32)      # every shift x both flips
    n = len(sf)
    assert n == 162
    index = rs.randint(N, size=n).astype(np.int32)                  # repeated and out of order
    index[:4] = [39, 0, 39, 17]
    at0 = int(np.flatnonzero((sf == 0).all(1))[0])
    dev = ctx.device
    with torch.cuda.stream(ctx.stream):
        d_img, d_lab = torch.from_numpy(images).to(dev), torch.from_numpy(labels_all).to(dev)
        d_idx, d_sf = torch.from_numpy(index).to(dev), torch.from_numpy(sf).to(dev)
        y = torch.full((n, 32, 32, 3), -1.0, dtype=torch.float32, device=dev)
        lab_out = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.rcgan_augment_cifar(ctx.h, n, N, d_img.data_ptr(), d_lab.data_ptr(), d_idx.data_ptr(), d_sf.data_ptr(), 4, L.F32,
                                          y.data_ptr(), lab_out.data_ptr()))
    ctx.sync()
    with torch.cuda.stream(ctx.stream):
        got, got_lab = y.cpu().numpy(), lab_out.cpu().numpy()
    ctx.sync()
    ref, ref_lab = R.augment(images, labels_all, index, sf)
    assert (got == ref).all(), int((got != ref).sum())
    assert (got_lab == ref_lab).all()
    # shift 0 without flip is the CHW -> NHWC transpose of the bytes
    assert (got[at0] == images[index[at0]].reshape(3, 32, 32).transpose(1, 2, 0).astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------ the other dispatch routes
def test_shortcut_a_misaligned_fp32_takes_the_scalar_route(ctx):
    """The float4 kernels need 16-byte aligned tensors; a caller of the C ABI that passes others gets the scalar kernels: same bits."""
    from rcgan_amd import _lib as L
    n, h, w, c = 2, 8, 8, 16
    rs = np.random.RandomState(4)
    x = rs.randn(n, h, w, c).astype(np.float32)
    dy = rs.randn(n, h // 2, w // 2, 2 * c).astype(np.float32)
    g0 = rs.randn(n, h, w, c).astype(np.float32)
    dev = ctx.device
    res = {}
    for off in (0, 1):                                   # element offset into a larger buffer: 0 = aligned, 1 = 4 bytes off
        with torch.cuda.stream(ctx.stream):
            bx = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
            bx[off:off + x.size].copy_(torch.from_numpy(x.reshape(-1)))
            bdy = torch.zeros(dy.size + 4, dtype=torch.float32, device=dev)
            bdy[off:off + dy.size].copy_(torch.from_numpy(dy.reshape(-1)))
            bdx = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
            bdx[off:off + x.size].copy_(torch.from_numpy(g0.reshape(-1)))
            by = torch.full((dy.size + 4,), -3.0, dtype=torch.float32, device=dev)
        ctx.check(ctx.lib.rcgan_shortcut_a_fwd(ctx.h, n, h, w, c, L.F32, bx.data_ptr() + 4 * off, by.data_ptr() + 4 * off))
        ctx.check(ctx.lib.rcgan_shortcut_a_bwd(ctx.h, n, h, w, c, L.F32, bdy.data_ptr() + 4 * off, bdx.data_ptr() + 4 * off, 1))
        ctx.sync()
        with torch.cuda.stream(ctx.stream):
            fy, fdx = by.cpu().numpy(), bdx.cpu().numpy()
        ctx.sync()
        # nothing outside the tensors is written
        assert (np.delete(fy, np.arange(off, off + dy.size)) == -3.0).all() and (np.delete(fdx, np.arange(off, off + x.size)) == 0).all()
        res[off] = (fy[off:off + dy.size].copy(), fdx[off:off + x.size].copy())
    assert (_bits(res[0][0]) == _bits(res[1][0])).all() and (_bits(res[0][1]) == _bits(res[1][1])).all()
    assert_close(res[1][0].reshape(dy.shape), _shortcut_ref(x), 2e-5, "misaligned forward")
    assert_close(res[1][1].reshape(x.shape), g0.astype(np.float64) + _shortcut_adj_ref(dy, c), 2e-5, "misaligned backward")


def test_shortcut_a_and_augment_in_16_bit_activations():
    """Both entry points dispatch on the activation dtype: bf16 here.  The shortcut stays the bits of meanpool2 + pad_channels; pixel
    values 0..255 are exact in bf16."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    from tests.gpu_util import bf16_round
    c16 = make_ctx("bf16")
    try:
        n, h, w, c = 2, 16, 16, 32
        rs = np.random.RandomState(6)
        x = bf16_round(rs.randn(n, h, w, c) * 3)
        c16.new_step()
        c16.recording = False
        xd = c16.upload(x)
        got = c16.download(O.shortcut_a(c16, xd))
        pooled = O.meanpool2(c16, xd)
        two = c16.empty((n, h // 2, w // 2, 2 * c))
        c16.check(c16.lib.rcgan_pad_channels(c16.h, n * (h // 2) * (w // 2), c, c // 2, c // 2, L.BF16, C.c_void_p(pooled.ptr), C.c_void_p(two.ptr)))
        assert (_bits(got) == _bits(c16.download(two))).all()
        assert_close(got, _shortcut_ref(x), 2.0 ** -8, "bf16 shortcut_a forward")          # one bf16 rounding of the result
        c16.recording = True
        dy = bf16_round(rs.randn(n, h // 2, w // 2, 2 * c))
        xd.req = True
        y = O.shortcut_a(c16, xd)
        y.grad = c16.upload(dy)
        c16.backward()
        assert (c16.download(xd.grad) == _shortcut_adj_ref(dy, c)).all()                     # a power of two times a bf16 value: exact
        # input pipeline
        N, m = 10, 12
        images = rs.randint(0, 256, size=(N, 3072)).astype(np.uint8)
        labels_all = rs.randint(20, size=N).astype(np.int32)
        index = rs.randint(N, size=m).astype(np.int32)
        sf = np.concatenate([rs.randint(-4, 5, size=(m, 2)), rs.randint(2, size=(m, 1))], axis=1).astype(np.int32)
        with torch.cuda.stream(c16.stream):
            d_img, d_lab = torch.from_numpy(images).to(c16.device), torch.from_numpy(labels_all).to(c16.device)
            d_idx, d_sf = torch.from_numpy(index).to(c16.device), torch.from_numpy(sf).to(c16.device)
            lab_out = torch.zeros(m, dtype=torch.int32, device=c16.device)
        yb = c16.empty((m, 32, 32, 3))
        c16.check(c16.lib.rcgan_augment_cifar(c16.h, m, N, d_img.data_ptr(), d_lab.data_ptr(), d_idx.data_ptr(), d_sf.data_ptr(), 4, L.BF16,
                                              C.c_void_p(yb.ptr), lab_out.data_ptr()))
        ref, ref_lab = R.augment(images, labels_all, index, sf)
        assert (c16.download(yb) == ref).all()
        with torch.cuda.stream(c16.stream):
            got_lab = lab_out.cpu().numpy()
        c16.sync()
        assert (got_lab == ref_lab).all()
    finally:
        c16.close()
