"""The "high" fp32 matmul precision (rcgan_set_f32_matmul_precision): the gather GEMM on split-bf16 matrix cores.

Op level: each output of the split route is compared with a float64 EMULATION of what it computes -- the oracle operation applied to
the three split-operand pairs (lo*hi + hi*lo + hi*hi, hi = bf16(x), lo = bf16(x - hi), after the ReLU-on-load, with the same
1/sigma) -- within TOL_EMUL of max|ref|.  Calibration (MI355X, these cases): the split route sits 0.9e-7..3.0e-7 of max|ref| from
its emulation -- fp32 accumulation of exact products over chains of at most ~300 (KS groups, split-R chunks); a float64 simulation of
sequential fp32 sums of 72..1152 exact products gives 2e-7..9e-7 -- while the exact-fp32 ("highest") route sits 3.7e-6..6.0e-6 from
it (the dropped lo*lo term and the bf16 rounding of lo: ~2^-16 of sum|a*b|).  TOL_EMUL = 1e-6 is ~3x from both, so every case also
asserts that "highest" FAILS it: the test tells the two routes apart and fails if the setting is ignored.
Inputs are random fp32 values, not bf16-representable (lo != 0)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import FakeParam, make_ctx

pytestmark = pytest.mark.gpu

TOL_EMUL = 1e-6       # split route vs its float64 emulation, of max|ref|
TOL_EXACT = 1e-4      # split route vs the exact float64 result, of max|ref|


def _split(a):
    a = np.asarray(a, np.float32)
    hi = torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()
    lo = torch.from_numpy(np.ascontiguousarray(a - hi)).bfloat16().float().numpy()
    return hi.astype(np.float64), lo.astype(np.float64)


def _pairs(a, b):
    """the three products the split route forms: (a_lo, b_hi), (a_hi, b_lo), (a_hi, b_hi)"""
    (ah, al), (bh, bl) = _split(a), _split(b)
    return [(al, bh), (ah, bl), (ah, bh)]


def _err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))


def _check(what, high, highest, emul, exact):
    e_high, e_highest, e_exact = _err(high, emul), _err(highest, emul), _err(high, exact)
    print("%-52s high-emulation %.2e  highest-emulation %.2e  high-exact %.2e" % (what, e_high, e_highest, e_exact))
    assert np.isfinite(high).all(), what
    assert e_high <= TOL_EMUL, "%s: high vs emulation %.3e > %.1e" % (what, e_high, TOL_EMUL)
    assert e_highest > TOL_EMUL, "%s: highest within the split tolerance (%.3e): the routes are not told apart" % (what, e_highest)
    assert e_exact <= TOL_EXACT, "%s: high vs exact %.3e > %.1e" % (what, e_exact, TOL_EXACT)


# ---- float64 convolutions (NHWC, HWIO filters, TF SAME padding) ------------------------------------------------------------------
def _pads(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2


def _conv(x, w, s):
    pt, pb = _pads(x.shape[1], w.shape[0], s)
    pl, pr = _pads(x.shape[2], w.shape[1], s)
    xt = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xt, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)


def _t(a, req=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=req)


def conv_fwd(x, w, s):
    return _conv(_t(x), _t(w), s).numpy()


def conv_dgrad(dy, w, xshape, s):
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    _conv(x, _t(w), s).backward(_t(dy))
    return x.grad.numpy()


def conv_wgrad(x, dy, wshape, s):
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    _conv(_t(x), w, s).backward(_t(dy))
    return w.grad.numpy()


def _up(a):
    return a.repeat(2, axis=1).repeat(2, axis=2)


def _pool_sum(a):
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32")
    yield c
    c.close()


def _conv_run(ctx, precision, x, wgt, b, sigma, dy, k, s, up, relu):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx.set_f32_matmul_precision(precision)
    ctx.new_step()
    xd = ctx.upload(x, L.F32)
    xd.req = True
    wp, bp = FakeParam(ctx, wgt), FakeParam(ctx, b)
    W = O.Weight(ctx, wp.t, ctx.upload(np.array([sigma], np.float32), L.F32))
    y = O.conv2d(ctx, xd, W, bp.t, k, s, in_up=up, in_relu=relu)
    out_y = ctx.download(y)
    y.grad = ctx.upload(dy, L.F32)
    ctx.backward()
    return out_y, ctx.download(xd.grad), ctx.download(W.dwbar)


# (n, h, w, cin, cout, k, stride, upsample-in, relu-in): which gather-GEMM launches they make (fwd / dgrad / wgrad)
CONV_CASES = [
    (2, 8, 8, 8, 16, 3, 1, True, True),        # KS = 1 everywhere; upsample-in, ReLU-on-load (+ its mask in the data gradient)
    (2, 8, 8, 128, 64, 3, 1, False, False),    # forward: split-R (4 chunks) at KS = 4; data gradient KS = 4; filter gradient KS = 1
    (32, 16, 16, 32, 128, 3, 1, False, True),  # forward KS = 2 (256 workgroups); data gradient KS = 4; filter gradient KS = 2
    (4, 14, 14, 16, 32, 5, 2, False, True),    # 5x5 stride 2: data gradient = DgradS2Op (four parity classes), masked
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_high_matches_split_emulation(ctx, case):
    n, h, w, cin, cout, k, s, up, relu = case
    rs = np.random.RandomState(1000 + CONV_CASES.index(case))
    hs, ws = (h // 2, w // 2) if up else (h, w)
    x = rs.randn(n, hs, ws, cin).astype(np.float32)
    wgt = (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32)
    b = (0.1 * rs.randn(cout)).astype(np.float32)
    sigma = np.float32(2.0)       # (a power of two: the prepared filter W / sigma is the same fp32 value however it is divided)
    oh, ow = -(-h // s), -(-w // s)
    dy = rs.randn(n, oh, ow, cout).astype(np.float32)
    hi = _conv_run(ctx, "high", x, wgt, b, sigma, dy, k, s, up, relu)
    hx = _conv_run(ctx, "highest", x, wgt, b, sigma, dy, k, s, up, relu)
    ctx.set_f32_matmul_precision("highest")
    # the operands as the kernels see them: ReLU-on-load, the nearest upsample, the prepared filter W / sigma (fp32)
    xin = np.maximum(x, 0) if relu else x
    xin = _up(xin) if up else xin
    w_eff = wgt / sigma
    xshape = (n, h, w, cin)
    y_emul = sum(conv_fwd(a, c, s) for a, c in _pairs(xin, w_eff)) + b
    y_exact = conv_fwd(xin, w_eff, s) + b
    dx_emul = sum(conv_dgrad(a, c, xshape, s) for a, c in _pairs(dy, w_eff))
    dx_exact = conv_dgrad(dy, w_eff, xshape, s)
    if up:
        dx_emul, dx_exact = _pool_sum(dx_emul), _pool_sum(dx_exact)
    if relu:
        dx_emul, dx_exact = dx_emul * (x > 0), dx_exact * (x > 0)
    dw_emul = sum(conv_wgrad(a, c, wgt.shape, s) for a, c in _pairs(xin, dy))
    dw_exact = conv_wgrad(xin, dy, wgt.shape, s)
    _check("conv fwd %s" % (case,), hi[0], hx[0], y_emul, y_exact)
    _check("conv dgrad %s" % (case,), hi[1], hx[1], dx_emul, dx_exact)
    _check("conv wgrad %s" % (case,), hi[2], hx[2], dw_emul, dw_exact)


def _dense_run(ctx, precision, x, wgt, sigma, dy):
    from rcgan_amd import _lib as L
    lib, h = ctx.lib, ctx.h
    m, k = x.shape
    n = wgt.shape[1]
    ctx.set_f32_matmul_precision(precision)
    ctx.new_step()
    xd, wd, dyd = ctx.upload(x, L.F32), ctx.upload(wgt, L.F32), ctx.upload(dy, L.F32)
    sg = ctx.upload(np.array([sigma], np.float32), L.F32)
    y, dx, dw = ctx.empty((m, n), L.F32), ctx.empty((m, k), L.F32), ctx.empty((k, n), L.F32)
    p = lambda t: C.c_void_p(t.ptr)
    ctx.check(lib.rcgan_linear_fwd(h, m, k, n, L.F32, p(xd), p(wd), p(sg), None, p(y)))
    ctx.check(lib.rcgan_linear_bwd_data(h, m, k, n, L.F32, p(dyd), p(wd), p(sg), p(dx), 0))
    ctx.check(lib.rcgan_linear_bwd_weight(h, m, k, n, L.F32, p(xd), p(dyd), p(dw), None, 0, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
    return ctx.download(y), ctx.download(dx), ctx.download(dw)


# (m, k, n): forward y[m,n] = x[m,k] W[k,n] / sigma, data gradient dx = dy W^T / sigma, filter gradient dW = x^T dy
DENSE_CASES = [
    (256, 1024, 512),     # forward KS = 4 (K-major x N-major); data gradient KS = 4 (K-major x K-major); filter gradient KS = 4 (N-major)
    (64, 1024, 8192),     # data gradient: split-R over the 8192-long reduction (8 chunks, KS = 4); filter gradient KS = 1
]


@pytest.mark.parametrize("case", DENSE_CASES)
def test_dense_high_matches_split_emulation(ctx, case):
    m, k, n = case
    rs = np.random.RandomState(2000 + DENSE_CASES.index(case))
    x = rs.randn(m, k).astype(np.float32)
    wgt = (rs.randn(k, n) / np.sqrt(k)).astype(np.float32)
    dy = rs.randn(m, n).astype(np.float32)
    sigma = np.float32(1.3)
    hi = _dense_run(ctx, "high", x, wgt, sigma, dy)
    hx = _dense_run(ctx, "highest", x, wgt, sigma, dy)
    ctx.set_f32_matmul_precision("highest")
    s = np.float64(sigma)
    _check("dense fwd %s" % (case,), hi[0], hx[0], sum(a @ c for a, c in _pairs(x, wgt)) / s, x.astype(np.float64) @ wgt / s)
    _check("dense dgrad %s" % (case,), hi[1], hx[1], sum(a @ c.T for a, c in _pairs(dy, wgt)) / s, dy.astype(np.float64) @ wgt.T / s)
    _check("dense wgrad %s" % (case,), hi[2], hx[2], sum(a.T @ c for a, c in _pairs(x, dy)), x.astype(np.float64).T @ dy)


def test_setter_rejects_unknown_values_and_highest_restores_the_exact_route(ctx):
    from rcgan_amd import _lib as L
    lib = ctx.lib
    assert lib.rcgan_set_f32_matmul_precision(ctx.h, -1) == -1
    assert lib.rcgan_set_f32_matmul_precision(ctx.h, 2) == -1
    rs = np.random.RandomState(7)
    x, wgt = rs.randn(256, 1024).astype(np.float32), (rs.randn(1024, 512) / 32).astype(np.float32)
    dy = rs.randn(256, 512).astype(np.float32)
    ctx.set_f32_matmul_precision("high")
    hi = _dense_run(ctx, "high", x, wgt, np.float32(1.0), dy)
    assert lib.rcgan_set_f32_matmul_precision(ctx.h, L.F32_PRECISION_HIGH) == 0
    assert lib.rcgan_set_f32_matmul_precision(ctx.h, L.F32_PRECISION_HIGHEST) == 0
    back = _dense_run(ctx, "highest", x, wgt, np.float32(1.0), dy)
    fresh_ctx = make_ctx("f32")
    try:
        fresh = _dense_run(fresh_ctx, "highest", x, wgt, np.float32(1.0), dy)
    finally:
        fresh_ctx.close()
    for a, f, h in zip(back, fresh, hi):
        assert np.array_equal(a, f)
        assert not np.array_equal(a, h)


# ---- step level --------------------------------------------------------------------------------------------------------------------
# || dP(high) - dP(highest) || / || dP(highest) || after one iteration, per weight tensor and over all parameters.  Adam's first updates
# are ~ +-lr per element, so an element whose gradient is below the routes' ~1e-5 relative difference can flip sign: measured (MI355X)
# 0.12 at most per tensor (the CIFAR generator's conditional batch-norm offsets), 0.04 over all CIFAR parameters, 0.004 for MNIST.
DELTA_TOL = 0.25


DELTA_TOL_ALL = 0.25


def _bias(name):
    # a bias in front of a batch norm has a zero gradient in exact arithmetic: its fp32 gradient is rounding noise and Adam's first
    # update moves it by +-lr whatever the noise is, so biases are compared only inside the all-parameter norm
    return name.lower().endswith(("biases", "bias", "/b"))


def _cifar_iteration(precision, use_graphs=True):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN, N_CRITIC
    rs = np.random.RandomState(31)
    B = 4
    C = np.linalg.inv(np.eye(10) * 0.6 + 0.4 / 10)
    ds = []
    for _ in range(N_CRITIC):
        lab = rs.randint(10, size=B)
        d = dict(images=rs.randint(0, 256, size=(B, 3072)), labels=lab, labels_random=rs.randint(10, size=B),
                 labels_biased=rs.randint(10, size=B), inv_weights=C[lab].astype(np.float32))
        d["labels_all"] = np.concatenate([d["labels"], d["labels_biased"]])
        ds.append(d)
    g = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="f32", seed=5, use_graphs=use_graphs, device_rng=True,
                   arena_bytes=2 << 30, f32_matmul_precision=precision)
    try:
        p0 = m.get_params()
        m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
        m.prepare_critic_fakes()
        m.critic_steps(ds, iteration=0)      # one captured graph of the five critic steps; eager: five d_step() calls
        d_loss, _ = m.losses()
        m.feed_host("g", **g)
        m.g_step(iteration=0)
        _, g_loss = m.losses()
        m.ctx.sync()
        p1 = m.get_params()
    finally:
        m.ctx.close()
    return (d_loss, g_loss), p0, p1


def _mnist_iteration(precision, use_graphs=True, iterations=1):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist import MnistRCGAN, create_variables
    rs = np.random.RandomState(37)
    B = 16
    eye = np.eye(10, dtype=np.float32)
    yr = rs.randint(10, size=B)
    b = dict(images=rs.rand(B, 28, 28, 1).astype(np.float32), z=rs.uniform(-1, 1, size=(B, 100)).astype(np.float32),
             y_real=eye[yr], y_gen=eye[rs.randint(10, size=B)], y_fake=eye[rs.randint(10, size=B)],
             y_real_weights=np.ones((B, 10), np.float32) * 0.1)
    variables = create_variables(0, "projection", True, True, True, ())
    m = MnistRCGAN(algorithm="rcgan", batch_size=B, dtype="f32", estimate_confuse=True, use_graphs=use_graphs, variables=variables,
                   f32_matmul_precision=precision)
    try:
        assert m.ctx.f32_matmul_precision == precision
        p0 = m.get_params()
        m.set_inputs(**b)
        for _ in range(iterations):
            m.iteration()
        losses = m.losses()
        p1 = m.get_params()
    finally:
        m.ctx.close()
    return losses, p0, p1


def _loss_values(losses):
    return [losses[k] for k in sorted(losses)] if isinstance(losses, dict) else list(losses)


def _compare_steps(what, a, b):
    (la, p0a, p1a), (lb, p0b, p1b) = a, b
    print("%s losses: high %s, highest %s" % (what, la, lb))
    for x, y in zip(_loss_values(la), _loss_values(lb)):
        assert abs(x - y) <= 1e-3 * max(abs(y), 1e-3), (what, la, lb)
    errs, num, den = {}, 0.0, 0.0
    for k in p0b:
        assert np.array_equal(p0a[k], p0b[k]), k
        da, db = p1a[k].astype(np.float64) - p0a[k], p1b[k].astype(np.float64) - p0b[k]
        if np.linalg.norm(db) == 0:
            assert np.linalg.norm(da) == 0, (what, k)
            continue
        num, den = num + float(np.sum((da - db) ** 2)), den + float(np.sum(db ** 2))
        if not _bias(k):
            errs[k] = float(np.linalg.norm(da - db) / np.linalg.norm(db))
    joint = (num / den) ** 0.5
    print("%s parameter-update differences: all parameters %.3e; largest weights %s" % (what, joint, sorted(errs.items(), key=lambda t: -t[1])[:6]))
    assert joint <= DELTA_TOL_ALL, (what, joint)
    for k, e in errs.items():
        assert e <= DELTA_TOL, (what, k, e)


def test_cifar_fp32_iteration_high_vs_highest():
    _compare_steps("cifar", _cifar_iteration("high"), _cifar_iteration("highest"))


def test_mnist_fp32_iteration_high_vs_highest():
    _compare_steps("mnist", _mnist_iteration("high"), _mnist_iteration("highest"))


def test_high_graph_replay_is_bit_identical_to_eager():
    # MNIST: capture on the first iteration, replays on the next two; CIFAR: the critic steps as one graph vs five eager steps
    (la, _, pa), (lb, _, pb) = _mnist_iteration("high", use_graphs=False, iterations=3), _mnist_iteration("high", iterations=3)
    assert la == lb
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    (la, _, pa), (lb, _, pb) = _cifar_iteration("high", use_graphs=False), _cifar_iteration("high")
    assert la == lb
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
