"""The kernels' routes for more than 16 classes (CIFAR-100, 1000-class sets), through the C ABI, against float64:
the conditional batch-norm backward (per-class dgamma / dbeta [K, c] and dx) and the projection head (loss, logits and every
gradient) for K in {17, 100, 1000}.  Tolerances are those of test_gpu_ops.py: 2e-5 of the reference's scale for fp32, the
storage-matched bounds for 16-bit activations.  Classes absent from the batch get exact zeros; repeated calls are bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import FakeParam, assert_close, half_round, make_ctx

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 1e-2, "f16": 3e-3}


@pytest.fixture(scope="module", params=["f32", "bf16", "f16"])
def dev(request):
    ctx = make_ctx(request.param)
    yield ctx, request.param
    ctx.close()


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _bn_run(ctx, x, labels, gamma, beta, dy, K, act, accumulate, prefill):
    """stats + apply + backward of the conditional batch norm; -> y, dx, dgamma, dbeta (host arrays)."""
    from rcgan_amd import _lib as L
    n, rps, c = x.shape
    xd = ctx.upload(x.reshape(n * rps, c), ctx.act_dtype)
    dyd = ctx.upload(dy.reshape(n * rps, c), ctx.act_dtype)
    yd = ctx.empty((n * rps, c), ctx.act_dtype)
    dxd = ctx.empty((n * rps, c), ctx.act_dtype)
    lab = ctx.upload(labels.astype(np.int32))
    gd, bd = ctx.upload(gamma, L.F32), ctx.upload(beta, L.F32)
    mean, rstd = ctx.empty((c,), L.F32), ctx.empty((c,), L.F32)
    dg, db = ctx.upload(prefill[0], L.F32), ctx.upload(prefill[1], L.F32)
    ws, wsb = C.c_void_p(ctx.ws_ptr), ctx.ws_bytes
    ctx.check(ctx.lib.rcgan_bn_stats(ctx.h, n * rps, c, xd.dtype, _p(xd), 1e-5, _p(mean), _p(rstd), None, None, 0.0, ws, wsb))
    ctx.check(ctx.lib.rcgan_bn_apply_fwd(ctx.h, n, rps, c, K, xd.dtype, _p(xd), _p(lab), _p(gd), _p(bd), _p(mean), _p(rstd), act, _p(yd),
                                         ws, wsb))
    ctx.check(ctx.lib.rcgan_bn_bwd2(ctx.h, n, rps, c, K, xd.dtype, _p(xd), _p(yd), _p(dyd), _p(lab), _p(gd), _p(bd), _p(mean), _p(rstd),
                                    act, _p(dxd), 0, _p(dg), _p(db), accumulate, ws, wsb))
    out = [ctx.download(t).astype(np.float64) for t in (yd, dxd, dg, db)]
    return out[0].reshape(n, rps, c), out[1].reshape(n, rps, c), out[2], out[3]


def _bn_ref(x, labels, gamma, beta, dy, mask):
    """float64: dgamma[l] = sum over class-l rows of dy' * xhat, dbeta[l] = sum dy', dx through the batch statistics."""
    n, rps, c = x.shape
    xr = x.reshape(-1, c).astype(np.float64)
    mu = xr.mean(0)
    rs = 1.0 / np.sqrt(xr.var(0) + 1e-5)
    xh = (xr - mu) * rs
    lr = np.repeat(labels, rps)
    g = dy.reshape(-1, c).astype(np.float64) * mask.reshape(-1, c)
    K = gamma.shape[0]
    dgam, dbet = np.zeros((K, c)), np.zeros((K, c))
    np.add.at(dgam, lr, g * xh)
    np.add.at(dbet, lr, g)
    dxh = g * gamma[lr].astype(np.float64)
    dx = rs * (dxh - dxh.mean(0) - xh * (dxh * xh).mean(0))
    y = xh * gamma[lr] + beta[lr]
    return y.reshape(n, rps, c), dx.reshape(n, rps, c), dgam, dbet


BN_CASES = [(K, c, n) for K in (17, 100, 1000) for c in (128, 256) for n in (4, 64, 128)]


@pytest.mark.parametrize("K,c,n", BN_CASES)
def test_cond_bn_many_classes(dev, K, c, n):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(K * 7 + c + n)
    rps = 16
    q = lambda a: half_round(mode, a)
    x = q(rs.randn(n, rps, c) * 1.5 + 0.3)
    dy = q(rs.randn(n, rps, c))
    gamma = (1.0 + 0.3 * rs.randn(K, c)).astype(np.float32)
    beta = (0.2 * rs.randn(K, c)).astype(np.float32)
    label_sets = {"random": rs.randint(K, size=n),                   # K = 100, 1000: most classes absent
                  "one": np.full(n, K - 1),                         # every sample in one class
                  "low": rs.randint(min(K, 3), size=n)}             # classes 3 .. K-1 absent
    for name, labels in label_sets.items():
        for acc in (0, 1):
            pre = [(rs.randn(K, c)).astype(np.float32) for _ in range(2)] if acc else [np.full((K, c), np.nan, np.float32)] * 2
            ctx.new_step()
            y, dx, dg, db = _bn_run(ctx, x, labels, gamma, beta, dy, K, L.ACT_NONE, acc, pre)
            yr, dxr, dgr, dbr = _bn_ref(x, labels, gamma, beta, dy, np.ones_like(x, np.float64))
            what = "K %d c %d n %d %s acc %d %s" % (K, c, n, name, acc, mode)
            tol = TOL[mode]
            assert_close(y, yr, tol, "y " + what)
            present = np.zeros(K, bool)
            present[labels] = True
            if acc:
                # absent classes keep their bits; present ones gain the reference
                assert np.array_equal(dg[~present], pre[0][~present].astype(np.float64)), what
                assert np.array_equal(db[~present], pre[1][~present].astype(np.float64)), what
                dg, db = dg - pre[0], db - pre[1]
            else:
                assert (dg[~present] == 0).all() and (db[~present] == 0).all(), "absent classes: exact zeros " + what
            # (fp32 sums of up to n*rps terms; the activation dy, x rounded on the host already)
            assert_close(dg[present], dgr[present], max(tol, 2e-5 if acc == 0 else 1e-4), "dgamma " + what)
            assert_close(db[present], dbr[present], max(tol, 2e-5 if acc == 0 else 1e-4), "dbeta " + what)
            assert_close(dx, dxr, tol if mode != "f32" else 1e-4, "dx " + what)


@pytest.mark.parametrize("K", [17, 100, 1000])
def test_cond_bn_many_classes_relu_and_repeat(dev, K):
    """ReLU with the mask recomputed from x (beta passed): the reference takes the mask of the GPU's own y; two calls on the
    same inputs give the same bits."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(K)
    n, rps, c = 64, 16, 256
    q = lambda a: half_round(mode, a)
    x, dy = q(rs.randn(n, rps, c)), q(rs.randn(n, rps, c))
    gamma = (1.0 + 0.3 * rs.randn(K, c)).astype(np.float32)
    beta = (0.2 * rs.randn(K, c)).astype(np.float32)
    labels = rs.randint(K, size=n)
    pre = [np.zeros((K, c), np.float32)] * 2
    ctx.new_step()
    a = _bn_run(ctx, x, labels, gamma, beta, dy, K, L.ACT_RELU, 0, pre)
    ctx.new_step()
    b = _bn_run(ctx, x, labels, gamma, beta, dy, K, L.ACT_RELU, 0, pre)
    for u, v in zip(a, b):
        assert np.array_equal(u, v), "repeat is not bit-identical"
    y, dx, dg, db = a
    _, dxr, dgr, dbr = _bn_ref(x, labels, gamma, beta, dy, (y > 0).astype(np.float64))
    tol = TOL[mode]
    assert_close(dg, dgr, max(tol, 2e-5), "dgamma relu")
    assert_close(db, dbr, max(tol, 2e-5), "dbeta relu")
    assert_close(dx, dxr, tol if mode != "f32" else 1e-4, "dx relu")


def test_bn_abi_bounds(dev):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    n, rps, c, K = 4, 16, 128, 1025
    t = ctx.empty((n * rps, c), ctx.act_dtype)
    f = ctx.empty((K * c,), L.F32)
    lab = ctx.upload(np.zeros(n, np.int32))
    rc = ctx.lib.rcgan_bn_bwd2(ctx.h, n, rps, c, K, t.dtype, _p(t), _p(t), _p(t), _p(lab), _p(f), _p(f), _p(f), _p(f), L.ACT_NONE, _p(t), 0,
                               _p(f), _p(f), 0, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes)
    assert rc != 0 and b"n_labels" in ctx.lib.rcgan_last_error(ctx.h)
    assert ctx.lib.rcgan_bn_workspace_bytes_labels(1024, 256, 16) == ctx.lib.rcgan_bn_workspace_bytes(1024, 256)
    assert ctx.lib.rcgan_bn_workspace_bytes_labels(1024, 256, 1000) > ctx.lib.rcgan_bn_workspace_bytes(1024, 256)


def test_bn_refuses_before_it_launches(dev):
    """Conditional calls without labels and empty shapes return EINVALID_ARG and leave the output as it was."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    n, rps, c, K = 4, 16, 128, 10
    x = ctx.upload(np.ones((n * rps, c), np.float32), ctx.act_dtype)
    f = ctx.upload(np.ones((K * c,), np.float32), L.F32)
    ws, wsb = C.c_void_p(ctx.ws_ptr), ctx.ws_bytes
    sentinel = -77.0
    y = ctx.upload(np.full((n * rps, c), sentinel, np.float32), ctx.act_dtype)
    mean, rstd = (ctx.upload(np.full((c,), sentinel, np.float32), L.F32) for _ in range(2))
    calls = {
        "apply_fwd without labels": lambda: ctx.lib.rcgan_bn_apply_fwd(ctx.h, n, rps, c, K, x.dtype, _p(x), None, _p(f), _p(f), _p(f), _p(f), L.ACT_NONE,
                                                                        _p(y), ws, wsb),
        "fwd_segments without labels": lambda: ctx.lib.rcgan_bn_fwd_segments(ctx.h, 2, n // 2, rps, c, K, x.dtype, _p(x), None, _p(f), _p(f), 1e-5,
                                                                              L.ACT_NONE, _p(mean), _p(rstd), _p(y), ws, wsb),
        "stats c = 0": lambda: ctx.lib.rcgan_bn_stats(ctx.h, n * rps, 0, x.dtype, _p(x), 1e-5, _p(mean), _p(rstd), None, None, 0.0, ws, wsb),
        "stats rows = 0": lambda: ctx.lib.rcgan_bn_stats(ctx.h, 0, c, x.dtype, _p(x), 1e-5, _p(mean), _p(rstd), None, None, 0.0, ws, wsb),
    }
    for what, call in calls.items():
        assert call() == L.EINVALID_ARG, what
        for t in (y, mean, rstd):
            assert (ctx.download(t) == sentinel).all(), what + ": output touched"


HEAD_PARTS = [
    ("HINGE_REAL", "lab", "HINGE_FAKE", "lab"),     # rcgan / biased critic step
    ("HINGE_REAL", "lab", "HINGE_FAKE", "wts"),     # rcgan-u critic step: confusion rows
    ("HINGE_REAL", "wts", "HINGE_FAKE", "lab"),     # unbiased: C^-1 rows
    ("NEG_MEAN", "wts", None, None),                # rcgan-u generator step
]


def _head(ctx, v, n, rows_a, parts_spec, rs, labels_hi=None):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    d, ed = 128, 300
    feat = rs.rand(n, d).astype(np.float32)
    w_out = (rs.randn(d, 1) * 0.3).astype(np.float32); b_out = rs.randn(1).astype(np.float32)
    table = (rs.randn(v, ed) * 0.1).astype(np.float32)
    w_e = (rs.randn(ed, d) * 0.2).astype(np.float32); b_e = (rs.randn(d) * 0.1).astype(np.float32)
    s_out, s_e, weight = np.float32(1.3), np.float32(0.7), 3.0
    kinds = {"HINGE_REAL": L.LOSS_HINGE_REAL, "HINGE_FAKE": L.LOSS_HINGE_FAKE, "NEG_MEAN": L.LOSS_NEG_MEAN}
    ctx.new_step()
    fd = ctx.upload(feat, L.F32); fd.req = True
    pw_out, pb_out, ptab, pw_e, pb_e = (FakeParam(ctx, a) for a in (w_out, b_out, table, w_e, b_e))
    W_out = O.Weight(ctx, pw_out.t, ctx.upload(np.array([s_out]), L.F32))
    W_e = O.Weight(ctx, pw_e.t, ctx.upload(np.array([s_e]), L.F32))
    ka, ma, kb, mb = parts_spec
    parts, host = [], []
    for rows, kind, md in ((rows_a, ka, ma), (n - rows_a, kb, mb)):
        if rows == 0:
            continue
        if md == "lab":
            lab = rs.randint(labels_hi or v, size=rows).astype(np.int32)
            parts.append((rows, kinds[kind], ctx.upload(lab), None)); host.append((rows, kind, lab, None, None))
        else:
            w = rs.rand(rows, v).astype(np.float32)
            wd = ctx.upload(w, L.F32); wd.req = True
            parts.append((rows, kinds[kind], None, wd)); host.append((rows, kind, None, w, wd))
    loss = ctx.persistent((1,), L.F32, fill=0.0)
    logits = ctx.empty((n, v), L.F32)
    O.proj_head(ctx, fd, W_out, pb_out.t, ptab.t, W_e, pb_e.t, parts, weight, loss, logits=logits)
    ctx.flush_wgrads()
    got = dict(loss=ctx.download(loss), logits=ctx.download(logits), dfeat=ctx.download(fd.grad), dw_out=ctx.download(W_out.dwbar),
               db_out=pb_out.grad(ctx), dtable=ptab.grad(ctx), dw_e=ctx.download(W_e.dwbar), db_e=pb_e.grad(ctx),
               dwts=[ctx.download(h[4].grad) for h in host if h[3] is not None])
    # float64 autograd restatement
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tf, two, tbo, tt, twe, tbe = T(feat), T(w_out), T(b_out), T(table), T(w_e), T(b_e)
    E = tt @ (twe / float(s_e)) + tbe
    psi = (tf @ (two / float(s_out))).reshape(-1) + tbo
    lg = psi[:, None] + tf @ E.t()
    total, r0, twts = 0.0, 0, []
    for rows, kind, lab, w, _ in host:
        x = lg[r0:r0 + rows]
        term = {"HINGE_REAL": torch.relu(1 - x), "HINGE_FAKE": torch.relu(1 + x), "NEG_MEAN": -x}[kind]
        if lab is not None:
            wt = torch.nn.functional.one_hot(torch.as_tensor(lab, dtype=torch.long), v).double()
        else:
            wt = T(w); twts.append(wt)
        total = total + (term * wt).sum(1).mean()
        r0 += rows
    total = weight * total
    total.backward()
    ref = dict(loss=np.array([float(total.detach())]), logits=lg.detach().numpy(), dfeat=tf.grad.numpy(),
               dw_out=two.grad.numpy() * float(s_out), db_out=tbo.grad.numpy(), dtable=tt.grad.numpy(),
               dw_e=twe.grad.numpy() * float(s_e), db_e=tbe.grad.numpy(), dwts=[w.grad.numpy() for w in twts])
    return got, ref, host


@pytest.mark.parametrize("v", [17, 100, 1000])
@pytest.mark.parametrize("spec", HEAD_PARTS)
def test_proj_head_many_classes(dev, v, spec):
    ctx, mode = dev
    if mode != "f32":
        pytest.skip("the head is fp32 regardless of the activation dtype")
    n = 32
    rows_a = n if spec[2] is None else 16
    rs = np.random.RandomState(v + len(spec[1]))
    got, ref, host = _head(ctx, v, n, rows_a, spec, rs)
    # (the weight-row parts sum v terms per sample: the loss and dwts at the bound of test_gpu_ops.py's head test)
    assert_close(got["loss"], ref["loss"], 1e-5, "head loss")
    r0 = 0
    for rows, kind, lab, w, _ in host:
        m = np.ones((rows, v), bool) if lab is None else (np.arange(v)[None] == lab[:, None])
        assert_close(got["logits"][r0:r0 + rows][m], ref["logits"][r0:r0 + rows][m], 2e-5, "head logits")
        r0 += rows
    for k in ("dfeat", "dw_out", "db_out", "dtable", "dw_e", "db_e"):
        assert_close(got[k], ref[k], 2e-5, "head " + k)
    for a, b in zip(got["dwts"], ref["dwts"]):
        assert_close(a, b, 2e-5, "head dwts")


def test_proj_head_absent_classes_and_repeat(dev):
    """One-hot parts that use classes 0..9 of 1000: the other 990 table rows get exact zeros; a second identical call gives
    the same bits."""
    ctx, mode = dev
    if mode != "f32":
        pytest.skip("the head is fp32 regardless of the activation dtype")
    spec = ("HINGE_REAL", "lab", "HINGE_FAKE", "lab")
    got, ref, _ = _head(ctx, 1000, 32, 16, spec, np.random.RandomState(5), labels_hi=10)
    again, _, _ = _head(ctx, 1000, 32, 16, spec, np.random.RandomState(5), labels_hi=10)
    assert (got["dtable"][10:] == 0).all()
    assert_close(got["dtable"], ref["dtable"], 2e-5, "head dtable")
    for k in ("loss", "logits", "dfeat", "dw_out", "db_out", "dtable", "dw_e", "db_e"):
        assert np.array_equal(got[k], again[k]), k


def test_proj_head_abi_bound(dev):
    from rcgan_amd import _lib as L
    ctx, mode = dev
    if mode != "f32":
        pytest.skip("one dtype is enough")
    n, d, v, ed = 8, 128, 1025, 300
    hd = L.HeadDesc(n, d, v, ed, n, L.LOSS_NEG_MEAN, 0, 1.0)
    lab = ctx.upload(np.zeros(n, np.int32))
    hd.labels_a = lab.ptr
    buf = ctx.empty((v * ed + ed * d + n * d,), L.F32)
    p = C.c_void_p(buf.ptr)
    rc = ctx.lib.rcgan_proj_head_fwd_bwd(ctx.h, C.byref(hd), p, p, None, p, p, p, None, p, p, None, None, None, None, None, None, None,
                                         C.c_void_p(ctx.ws_ptr), ctx.ws_bytes)
    assert rc != 0 and b"head shape" in ctx.lib.rcgan_last_error(ctx.h)
