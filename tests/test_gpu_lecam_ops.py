"""The regularised loss entry points (rcgan_loss_reg_fwd_bwd, rcgan_proj_head_reg_fwd_bwd; csrc/loss.hip) through ctypes, between
guard bands (tests/guard.py), against float64 references: tests/lecam_ref.py for the unfused kernel, float64 autograd of the same
formulas for the fused head.

Exact checks: a closed gate, lambda = 0 or no descriptor give the plain entry point's bits on every output (and leave reg_acc alone);
a second run gives the first one's bits; with every hinge inactive the unfused dlogit is the regulariser's term evaluated in fp32 in
the kernel's order, and the head's plain call leaves exact zeros where the regularised one leaves the regulariser's gradient.

Bounds of the unfused kernel, from the reference's own terms (head_loss_ref.sum_bound / elem_bound):
  dlogit = gw wf (loss' + 2 lambda (x - a)): x - a is one correctly rounded subtraction of two fp32 inputs, the bracket a two-term sum,
      the rest products -- elem_bound + sum_bound(2, .) of mag = |gw wf| (|loss'| + |2 lambda (x - a)|); dwts likewise of
      |gw / rows| (|loss| + |lambda (x - a)^2|).
  loss_acc: N = rows * cols terms (+ the accumulator's old value), each carrying at most eight roundings beyond its place in the sum
      (the loss term's own three, x - a, its square, the product with lambda, the weight factor, the products with it):
      sum_bound(N + 8, sum|terms|).  reg_acc: the same with four (x - a, the square, the weight factor, the product): sum_bound(N + 4, .).
The fused head's outputs take the bounds of the existing fused-head cases for the same outputs (tests/test_gpu_ops.py::test_proj_head,
tests/test_gpu_many_classes_ops.py: 1e-5 of max|ref| on the loss, 2e-5 on logits and every gradient, TOL[mode] on a 16-bit dx): the
reductions behind them are unchanged.  reg_acc is reduced exactly as the loss is: 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import head_loss_ref as R
from tests import lecam_ref as LR
from tests.gpu_util import FakeParam, assert_close, half_round, make_ctx
from tests.guard import guarded
from tests.test_gpu_ops import TOL

pytestmark = pytest.mark.gpu

LAM, A_R, A_F = 0.3, -0.8, 0.6


@pytest.fixture(scope="module")
def _contexts():
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx, arena_bytes=256 << 20, ws_bytes=32 << 20)
            ctx.guard = cm.__enter__()
            made[mode] = (ctx, cm)
        made[mode][0].guard.clear()
        return made[mode][0]

    yield get
    for ctx, cm in made.values():
        cm.__exit__(None, None, None)
        ctx.close()


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _state(ctx, gate):
    """The anchors as the engine lays them out: {a_R, a_F, updates = the gate, ...}."""
    from rcgan_amd import _lib as L
    return ctx.upload(np.array([A_R, A_F, gate, 0, 0, 0, 0, 0], np.float32), dtype=L.F32)


# ---------------------------------------------------------------------------------------------- the unfused kernel
UNFUSED = [(1, 1, False), (3, 1, False), (257, 1, False), (64, 10, False), (64, 10, True), (5, 100, True)]       # rows, cols, weights
OPTIONS = [(1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (0, 0, 1, 1), (1, 1, 0, 0)]                                  # dlogit, dwts, loss_acc, reg_acc set


def _unfused(ctx, kind, x, wts, weight, reg, opts=(1, 1, 1, 1), acc0=(1.5, 0.25), racc=None):
    """One call; -> dict of the outputs that were asked for (device tensors) and the untouched ones."""
    from rcgan_amd import _lib as L
    rows, cols = x.shape
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    xd, wd = up(x), (up(wts) if wts is not None else None)
    dx, dw = ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32)
    loss = up([acc0[0]]) if opts[2] else ctx.empty((1,), L.F32)
    if reg is not None and racc is None:
        racc = up([acc0[1]]) if opts[3] else None
    if reg is not None:
        reg = L.LossReg(reg[0], reg[1], None, reg[2], racc.ptr if racc is not None else None)
    ctx.check(ctx.lib.rcgan_loss_reg_fwd_bwd(ctx.h, kind, rows, cols, _p(xd), _p(wd), weight, _p(loss) if opts[2] else None,
                                             _p(dx) if opts[0] else None, _p(dw) if opts[1] else None, C.byref(reg) if reg is not None else None))
    return dict(dlogit=dx, dwts=dw, loss=loss, racc=racc)


def _unfused_inputs(rs, kind, rows, cols, weighted):
    x = (rs.randn(rows, cols) * 2).astype(np.float32)
    if kind in (R.HINGE_REAL, R.HINGE_FAKE) and rows * cols >= 3:
        x.reshape(-1)[::3] = 1.0 if kind == R.HINGE_REAL else -1.0        # exactly at the kink: term and derivative 0
    w = None
    if weighted:                                                          # rows that sum to 1, negative entries among them (C^-1 rows)
        w = rs.randn(rows, cols)
        w = (w + (1.0 - w.sum(1, keepdims=True)) / cols).astype(np.float32)
        assert (w < 0).any()
    return x, w


@pytest.mark.parametrize("kind", [R.HINGE_REAL, R.HINGE_FAKE, R.NEG_MEAN, R.CE_ONES, R.CE_ZEROS])
def test_unfused_kernel_against_the_float64_reference(_contexts, kind):
    ctx = _contexts("f32")
    g = ctx.guard
    rs = np.random.RandomState(40 + kind)
    weight = -2.0 if kind == R.NEG_MEAN else 1.7
    todo = []
    for i, (rows, cols, weighted) in enumerate(UNFUSED):
        x, w = _unfused_inputs(rs, kind, rows, cols, weighted)
        st = _state(ctx, 3.0)
        a = A_F if kind != R.HINGE_FAKE else A_R
        anchor = st.ptr + (4 if kind != R.HINGE_FAKE else 0)
        ref = LR.loss_reg_fwd_bwd(kind, x, w, weight, np.float32(LAM), np.float32(a), 3.0)
        for opts in (OPTIONS[i % 5], OPTIONS[(i + 1) % 5], OPTIONS[0]):
            out = _unfused(ctx, kind, x, w, weight, (LAM, anchor, st.ptr + 8), opts)
            todo.append(("kind %d %dx%d wts %d opts %r" % (kind, rows, cols, weighted, opts), out, opts, ref, rows * cols))
    ctx.sync()
    g.check()
    for what, out, opts, ref, N in todo:
        for key, on in (("dlogit", opts[0]), ("dwts", opts[1])):
            if not on:
                assert g.unwritten(out[key]) == out[key].size, what + ": a skipped output was written"
                continue
            mag = ref[key + "_mag"]
            wr = R.worst(ctx.download(out[key]), ref[key], R.elem_bound(mag) + R.sum_bound(2, mag))
            assert wr <= 1.0, "%s %s: worst error / bound %.3g" % (what, key, wr)
        if opts[2]:
            wr = R.worst(ctx.download(out["loss"]), np.array([1.5 + ref["value"]]), R.sum_bound(N + 1 + 8, 1.5 + ref["mag"]))
            assert wr <= 1.0, "%s loss: worst error / bound %.3g" % (what, wr)
        else:
            assert g.unwritten(out["loss"]) == 1, what
        if opts[3]:
            wr = R.worst(ctx.download(out["racc"]), np.array([0.25 + ref["R"]]), R.sum_bound(N + 1 + 4, 0.25 + ref["R_mag"]))
            assert wr <= 1.0, "%s reg_acc: worst error / bound %.3g" % (what, wr)


@pytest.mark.parametrize("kind", [R.HINGE_REAL, R.HINGE_FAKE, R.CE_ONES])
def test_unfused_kernel_off_is_the_plain_entry_point_and_a_repeat_has_the_same_bits(_contexts, kind):
    from rcgan_amd import _lib as L
    ctx = _contexts("f32")
    rs = np.random.RandomState(60 + kind)
    for rows, cols, weighted in UNFUSED:
        x, w = _unfused_inputs(rs, kind, rows, cols, weighted)
        up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
        xd, wd = up(x), (up(w) if weighted else None)
        dx, dw, loss = ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32), up([1.5])
        ctx.check(ctx.lib.rcgan_loss_fwd_bwd(ctx.h, kind, rows, cols, _p(xd), _p(wd), 1.7, _p(loss), _p(dx), _p(dw)))
        plain = [ctx.download(t) for t in (dx, dw, loss)]
        open_, shut = _state(ctx, 1.0), _state(ctx, 0.0)
        offs = [None, (LAM, shut.ptr + 4, shut.ptr + 8), (0.0, open_.ptr + 4, open_.ptr + 8), (0.0, open_.ptr + 4, None)]
        for reg in offs:
            out = _unfused(ctx, kind, x, w, 1.7, reg)
            for name, t, want in zip(("dlogit", "dwts", "loss"), (out["dlogit"], out["dwts"], out["loss"]), plain):
                assert np.array_equal(_bits(ctx.download(t)), _bits(want)), (kind, rows, cols, reg, name)
            if reg is not None:
                assert np.array_equal(_bits(ctx.download(out["racc"])), _bits([0.25])), "a closed gate moved reg_acc"
        # on (also with no gate word at all: always on): two runs, the same bits, and not the plain ones
        for reg in ((LAM, open_.ptr + 4, open_.ptr + 8), (LAM, open_.ptr + 4, None)):
            a, b = _unfused(ctx, kind, x, w, 1.7, reg), _unfused(ctx, kind, x, w, 1.7, reg)
            for name in ("dlogit", "dwts", "loss", "racc"):
                assert np.array_equal(_bits(ctx.download(a[name])), _bits(ctx.download(b[name]))), (kind, rows, cols, name)
            assert not np.array_equal(_bits(ctx.download(a["dlogit"])), _bits(plain[0]))
    ctx.sync()
    ctx.guard.check()


def test_unfused_inactive_hinges_leave_exactly_the_regularisers_term(_contexts):
    """Real logits > 1, fake logits < -1: the plain dlogit is all zeros, the regularised one is gw * (2 lambda (x - a)) * wf evaluated
    in fp32 in the kernel's order (the kernel's 0 + 2 lambda (x - a), fused or not, is the rounded product)."""
    from rcgan_amd import _lib as L
    ctx = _contexts("f32")
    rs = np.random.RandomState(7)
    f = np.float32
    for kind, sign, a, off in ((R.HINGE_REAL, 1.0, A_F, 4), (R.HINGE_FAKE, -1.0, A_R, 0)):
        for rows, cols, weighted in UNFUSED:
            x = (sign * (1.0 + 1e-3 + np.abs(rs.randn(rows, cols)) * 3)).astype(np.float32)
            _, w = _unfused_inputs(rs, kind, rows, cols, weighted)
            st = _state(ctx, 2.0)
            up = lambda v: ctx.upload(np.asarray(v, np.float32), L.F32)
            dx = ctx.empty((rows, cols), L.F32)
            ctx.check(ctx.lib.rcgan_loss_fwd_bwd(ctx.h, kind, rows, cols, _p(up(x)), _p(up(w)) if weighted else None, 1.7, None, _p(dx), None))
            assert not ctx.download(dx).any(), "an inactive hinge has a gradient"
            out = _unfused(ctx, kind, x, w, 1.7, (LAM, st.ptr + off, st.ptr + 8), (1, 0, 0, 0))
            u = x - f(a)
            d = (f(2.0) * f(LAM)) * u
            inv_rows, inv_all = f(1.0) / f(rows), f(1.0) / f(rows * cols)
            wf = w * inv_rows if weighted else inv_all
            want = (f(1.7) * d) * wf
            assert np.array_equal(_bits(ctx.download(out["dlogit"])), _bits(want)), (kind, rows, cols, weighted)
    ctx.sync()
    ctx.guard.check()


def test_unfused_bad_descriptors_are_refused_before_anything_is_launched(_contexts):
    from rcgan_amd import _lib as L
    ctx = _contexts("f32")
    g = ctx.guard
    x = ctx.upload(np.ones((4, 1), np.float32), L.F32)
    st = _state(ctx, 1.0)
    dx = ctx.empty((4, 1), L.F32)
    for reg in (L.LossReg(-0.5, st.ptr, None, st.ptr + 8, None), L.LossReg(float("nan"), st.ptr, None, st.ptr + 8, None),
                L.LossReg(float("inf"), st.ptr, None, st.ptr + 8, None), L.LossReg(LAM, None, None, st.ptr + 8, None),
                L.LossReg(LAM, st.ptr + 2, None, st.ptr + 8, None), L.LossReg(LAM, st.ptr, None, st.ptr + 9, None),
                L.LossReg(LAM, st.ptr, None, st.ptr + 8, st.ptr + 21)):
        rc = ctx.lib.rcgan_loss_reg_fwd_bwd(ctx.h, R.HINGE_REAL, 4, 1, _p(x), None, 1.0, None, _p(dx), None, C.byref(reg))
        assert rc == L.EINVALID_ARG
    ctx.sync()
    g.check()
    assert g.unwritten(dx) == 4


# ---------------------------------------------------------------------------------------------- the fused head
class _NullDescriptor:
    """ctx.lib with the plain head call sent to the regularised entry point without a descriptor."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def rcgan_proj_head_fwd_bwd(self, *a):
        return self._lib.rcgan_proj_head_reg_fwd_bwd(*a, None)


KIND_NAMES = {"HINGE_REAL": R.HINGE_REAL, "HINGE_FAKE": R.HINGE_FAKE}
SPECS = [("lab", "lab"), ("lab", "wts"), ("wts", "lab")]


def _head_data(rs, v, n, rows_a, spec, inactive=False, x_hw=None, mode="f32"):
    d, ed = 128, 300
    D = dict(v=v, n=n, rows_a=rows_a, d=d, ed=ed)
    sign = np.where(np.arange(n) < rows_a, 1.0, -1.0)[:, None]
    if x_hw:
        D["x"] = half_round(mode, rs.randn(n, x_hw, 1, d).astype(np.float32))
    else:
        D["feat"] = (sign * (rs.rand(n, d) + 0.5)).astype(np.float32) if inactive else rs.rand(n, d).astype(np.float32)
    D["w_out"] = ((np.abs(rs.randn(d, 1)) * 0.3 + 0.1) if inactive else rs.randn(d, 1) * 0.3).astype(np.float32)
    D["b_out"] = (rs.randn(1) * (0.1 if inactive else 1.0)).astype(np.float32)
    D["table"] = (rs.randn(v, ed) * (0.01 if inactive else 0.1)).astype(np.float32)
    D["w_e"] = (rs.randn(ed, d) * 0.2).astype(np.float32)
    D["b_e"] = (rs.randn(d) * (0.01 if inactive else 0.1)).astype(np.float32)
    D["parts"] = []
    for rows, kind, md in ((rows_a, "HINGE_REAL", spec[0]), (n - rows_a, "HINGE_FAKE", spec[1])):
        if rows == 0:
            continue
        if md == "lab":
            D["parts"].append((rows, kind, rs.randint(v, size=rows).astype(np.int32), None))
        else:
            w = rs.randn(rows, v)
            D["parts"].append((rows, kind, None, (w + (1.0 - w.sum(1, keepdims=True)) / v).astype(np.float32)))
    return D


S_OUT, S_E, WEIGHT = np.float32(1.3), np.float32(0.7), 3.0


def _head_run(ctx, D, how):
    """how: "plain" | "absent" | "shut" | "lam0" | "on".  -> dict of numpy outputs."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx.new_step()
    n, v, d = D["n"], D["v"], D["d"]
    pw_out, pb_out, ptab, pw_e, pb_e = (FakeParam(ctx, D[k]) for k in ("w_out", "b_out", "table", "w_e", "b_e"))
    W_out = O.Weight(ctx, pw_out.t, ctx.upload(np.array([S_OUT]), L.F32))
    W_e = O.Weight(ctx, pw_e.t, ctx.upload(np.array([S_E]), L.F32))
    if "x" in D:
        xd = ctx.upload(D["x"]); xd.req = True
        feat = O.act_meanhw_later(ctx, xd, L.ACT_RELU)
        assert isinstance(feat, O.PooledLater)
    else:
        feat = ctx.upload(D["feat"], L.F32); feat.req = True
    parts, wds = [], []
    for rows, kind, lab, w in D["parts"]:
        if lab is not None:
            parts.append((rows, KIND_NAMES[kind], ctx.upload(lab), None))
        else:
            wd = ctx.upload(w, L.F32); wd.req = True
            wds.append(wd)
            parts.append((rows, KIND_NAMES[kind], None, wd))
    loss = ctx.persistent((1,), L.F32, fill=0.5)
    racc = ctx.persistent((1,), L.F32, fill=0.25)
    logits = ctx.empty((n, v), L.F32)
    st = _state(ctx, 0.0 if how == "shut" else 2.0)
    reg = None
    if how in ("shut", "lam0", "on"):
        reg = O.lecam_reg(0.0 if how == "lam0" else LAM, st.ptr + 4, st.ptr if len(parts) > 1 else None, st.ptr + 8, racc.ptr)
    lib = ctx.lib
    try:
        if how == "absent":
            ctx.lib = _NullDescriptor(lib)
        O.proj_head(ctx, feat, W_out, pb_out.t, ptab.t, W_e, pb_e.t, parts, WEIGHT, loss, logits=logits, reg=reg)
    finally:
        ctx.lib = lib
    ctx.flush_wgrads()
    ctx.sync()
    ctx.guard.check()
    out = dict(loss=ctx.download(loss), racc=ctx.download(racc), logits=ctx.download(logits), dw_out=ctx.download(W_out.dwbar),
               db_out=pb_out.grad(ctx), dtable=ptab.grad(ctx), dw_e=ctx.download(W_e.dwbar), db_e=pb_e.grad(ctx),
               dwts=[ctx.download(w.grad) for w in wds])
    out["dx" if "x" in D else "dfeat"] = ctx.download(xd.grad if "x" in D else feat.grad)
    return out


def _head_ref(D, lam):
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    two, tbo, tt, twe, tbe = (T(D[k]) for k in ("w_out", "b_out", "table", "w_e", "b_e"))
    if "x" in D:
        tin = T(D["x"])
        tf = torch.relu(tin).mean(dim=(1, 2))
    else:
        tin = tf = T(D["feat"])
    v = D["v"]
    E = tt @ (twe / float(S_E)) + tbe
    lg = ((tf @ (two / float(S_OUT))).reshape(-1) + tbo)[:, None] + tf @ E.t()
    total, Rsum, r0, twts, masks = 0.0, 0.0, 0, [], []
    for (rows, kind, lab, w), a in zip(D["parts"], (float(np.float32(A_F)), float(np.float32(A_R)))):
        x = lg[r0:r0 + rows]
        term = torch.relu(1 - x) if kind == "HINGE_REAL" else torch.relu(1 + x)
        q = (x - a) ** 2
        if lab is not None:
            wt = torch.nn.functional.one_hot(torch.as_tensor(lab, dtype=torch.long), v).double()
            masks.append(np.arange(v)[None] == lab[:, None])
        else:
            wt = T(w); twts.append(wt)
            masks.append(np.ones((rows, v), bool))
        total = total + ((term + lam * q) * wt).sum(1).mean()
        Rsum = Rsum + (q * wt).sum(1).mean()
        r0 += rows
    total = WEIGHT * total
    total.backward()
    ref = dict(loss=np.array([0.5 + float(total.detach())]), racc=np.array([0.25 + float(Rsum.detach())]), logits=lg.detach().numpy(),
               dw_out=two.grad.numpy() * float(S_OUT), db_out=tbo.grad.numpy(), dtable=tt.grad.numpy(), dw_e=twe.grad.numpy() * float(S_E),
               db_e=tbe.grad.numpy(), dwts=[w.grad.numpy() for w in twts], mask=np.concatenate(masks, 0))
    ref["dx" if "x" in D else "dfeat"] = tin.grad.numpy()
    return ref


def _same_bits(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        if k == "dwts":
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[k], b[k])), (what, k)
        else:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _head_close(got, ref, what, dx_tol=2e-5):
    assert_close(got["loss"], ref["loss"], 1e-5, what + " loss")
    assert_close(got["racc"], ref["racc"], 1e-5, what + " reg_acc")
    assert_close(got["logits"][ref["mask"]], ref["logits"][ref["mask"]], 2e-5, what + " logits")
    for k in ("dfeat", "dw_out", "db_out", "dtable", "dw_e", "db_e"):
        if k in got:
            assert_close(got[k], ref[k], 2e-5, what + " " + k)
    if "dx" in got:
        assert_close(got["dx"], ref["dx"], dx_tol, what + " dx")
    for a, b in zip(got["dwts"], ref["dwts"]):
        assert_close(a, b, 2e-5, what + " dwts")


HEAD_SHAPES = [(1, 1), (5, 2), (128, 64)]                    # n, rows_a


@pytest.mark.parametrize("v", [1, 10, 16, 17, 100])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head(_contexts, v, shape):
    """Both routes (v <= 16: label embeddings in LDS; v > 16: the wide route) and their boundary; one part, an odd split, a full grid."""
    ctx = _contexts("f32")
    n, rows_a = shape
    spec = SPECS[(v + n) % 3]
    D = _head_data(np.random.RandomState(100 * v + n), v, n, rows_a, spec)
    what = "head v %d n %d rows_a %d %r" % (v, n, rows_a, spec)
    plain = _head_run(ctx, D, "plain")
    for how in ("absent", "shut", "lam0"):
        _same_bits(plain, _head_run(ctx, D, how), what + " " + how)          # (reg_acc too: still its 0.25)
    on = _head_run(ctx, D, "on")
    _same_bits(on, _head_run(ctx, D, "on"), what + " repeat")
    _head_close(on, _head_ref(D, LAM), what)
    _head_close(plain, dict(_head_ref(D, 0.0), racc=np.array([0.25])), what + " plain")
    assert not np.array_equal(_bits(on["dfeat"]), _bits(plain["dfeat"]))


@pytest.mark.parametrize("v", [10, 100])
@pytest.mark.parametrize("spec", SPECS)
def test_fused_head_with_every_hinge_inactive(_contexts, v, spec):
    """Real logits > 1 and fake logits < -1 for every label: the plain head back-propagates exact zeros -- the failure the regulariser
    is there for -- and the regularised head the regulariser's own gradient."""
    ctx = _contexts("f32")
    D = _head_data(np.random.RandomState(v + len(spec[0])), v, 16, 8, spec, inactive=True)
    ref = _head_ref(D, LAM)
    lg = ref["logits"]
    assert (lg[:8] > 1.001).all() and (lg[8:] < -1.001).all(), "the case must keep every hinge inactive"
    plain = _head_run(ctx, D, "plain")
    for k in ("dfeat", "dw_out", "db_out", "dtable", "dw_e", "db_e"):
        assert not plain[k].any(), "plain head, inactive hinges: %s is not zero" % k
    assert plain["loss"][0] == 0.5
    on = _head_run(ctx, D, "on")
    _head_close(on, ref, "inactive hinges v %d %r" % (v, spec))
    assert on["dfeat"].any(axis=1).all(), "a row without a gradient"


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_fused_head_pooling_from_16_bit_activations(_contexts, mode):
    ctx = _contexts(mode)
    D = _head_data(np.random.RandomState(5), 10, 5, 2, ("lab", "lab"), x_hw=64, mode=mode)
    plain = _head_run(ctx, D, "plain")
    _same_bits(plain, _head_run(ctx, D, "shut"), "pooled head, closed gate")
    on = _head_run(ctx, D, "on")
    _same_bits(on, _head_run(ctx, D, "on"), "pooled head repeat")
    _head_close(on, _head_ref(D, LAM), "pooled head " + mode, dx_tol=TOL[mode])
