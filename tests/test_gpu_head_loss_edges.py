"""The unfused head, loss and softmax kernels of csrc/loss.hip and rcgan_bn_infer / rcgan_bn_infer_bwd at their edges, through the C ABI,
against the float64 references of tests/head_loss_ref.py, inside guard bands (tests/guard.py).

Shapes: sizes that are no multiple of the lane / tile / block width, more than one block, one case per grid-stride kernel past the
4096-block grid cap; every accumulate flag both ways; every optional pointer NULL and non-NULL; the gradient scale of
rcgan_set_grad_scale applied; logits of the sigmoid cross-entropy out to +-80.

Tolerances (none tuned against the kernels; derivations in tests/head_loss_ref.py):
  elementwise results in fp32   |got - ref| <= 1e-5 |ref| + 1e-37 per element (R.elem_bound)
  sums of L terms               |got - ref| <= (L + 4) 2^-24 sum|terms| per element (R.sum_bound), sum|terms| from the fp64 reference
  an fp32 value added onto one  the elementwise bound of the new value + the two-term sum bound
  outputs stored in 16 bits     TOL[mode] of test_gpu_ops.py relative to max|ref|, inputs rounded to the format first
  exact results                 bitwise: gather, absent scatter rows, skipped outputs, repeated runs, the x512 of the gradient scale

Every case is launched into fresh 0xFF-filled outputs; after ctx.sync(): Guard.check(), no output element still holds the fill, an output
the call was told to skip still holds all of it.  One case per entry point runs twice and must give the same bits (no floating-point
atomics anywhere in these kernels).

On the kernels before the sigmoid gradient was rewritten (1 / (1 + expf(-x)) - z) the saturated cases fail on an MI355X:
test_loss_fwd_bwd[CE_ONES] at 90 x its bound on the first case, test_bce_onehot_fwd_bwd at 46 x, test_fused_head_saturated_logits
[CE_ONES, v = 10 and 17] with dfeat 13 % off where 1e-4 is asked; CE_ZEROS was cancellation-free already and passes on both.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import head_loss_ref as R
from tests.guard import guarded
from tests.gpu_util import assert_close, half_round, make_ctx
from tests.test_gpu_ops import TOL

pytestmark = pytest.mark.gpu

EPS32 = R.EPS32
SAT = (10.0, 12.0, 17.0, 30.0, 80.0)


@pytest.fixture(scope="module")
def _contexts():
    """One guarded context per activation dtype, made on first use and kept for the module."""
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx, arena_bytes=512 << 20, ws_bytes=32 << 20)
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


@pytest.fixture(scope="module")
def dev32(_contexts):
    """The fp32-only entry points run once."""
    return _contexts("f32")


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _added(new, prev):
    """Bound of fp32 `new + prev` where `new` is an elementwise result: its own bound + the two-term sum bound."""
    return R.elem_bound(new) + R.sum_bound(2, np.abs(new) + np.abs(prev))


class Batch:
    """Launch many small cases, judge them after ONE sync: bands first, then every output."""

    def __init__(self, ctx):
        self.ctx, self.g, self.todo = ctx, ctx.guard, []
        self.g.clear()

    def close(self, what, t, ref, bound):
        self.todo.append((what, t, lambda got: R.worst(got, ref, bound) <= 1.0, lambda got: "worst error / bound %.3g" % R.worst(got, ref, bound)))

    def half(self, what, t, ref, mode):
        """An output stored in 16 bits (or fp32 under the same case list): TOL[mode] of max|ref|."""
        self.todo.append((what, t, lambda got: (assert_close(got, ref, TOL[mode], what), True)[1], lambda got: ""))

    def bits(self, what, t, ref):
        self.todo.append((what, t, lambda got: np.array_equal(_bits(got), _bits(ref)), lambda got: "bits differ"))

    def same(self, what, t, u):
        self.todo.append((what, t, lambda got: np.array_equal(_bits(got), _bits(self.ctx.download(u))), lambda got: "two runs differ"))

    def where(self, what, t, fn):
        self.todo.append((what, t, fn, lambda got: "property does not hold"))

    def untouched(self, what, t):
        self.todo.append((what, t, None, None))

    def done(self):
        ctx, g = self.ctx, self.g
        ctx.sync()
        g.check()
        for what, t, ok, why in self.todo:
            if ok is None:
                assert g.unwritten(t) == t.size, what + ": a skipped output was written"
                continue
            assert g.unwritten(t) == 0, "%s: %d elements never written" % (what, g.unwritten(t))
            got = ctx.download(t)
            assert ok(got), "%s: %s" % (what, why(got))
        self.todo = []
        ctx.new_step()


def _with_zeros(rs, shape, scale=1.5):
    x = rs.randn(*shape) * scale
    x.reshape(-1)[::7] = 0.0
    return x


# ---------------------------------------------------------------------------------------------------- act_meanhw
@pytest.mark.parametrize("n", [1, 3])
def test_act_meanhw(dev, n):
    """4 row lanes x 64 columns per workgroup, grid (ceil(c / 64), n): c and hw around the lane counts; exact zeros in x."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    B = Batch(ctx)
    rs = np.random.RandomState(100 + n)
    for hw, c in itertools.product((1, 3, 4, 5, 49, 64), (1, 63, 64, 65, 130)):
        x = half_round(mode, _with_zeros(rs, (n, hw, c)))
        dfeat = rs.randn(n, c).astype(np.float32)
        xd, dfd = ctx.upload(x), ctx.upload(dfeat, L.F32)
        for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU):
            what = "act_meanhw n %d hw %d c %d act %d %s" % (n, hw, c, act, mode)
            feat, dx = ctx.empty((n, c), L.F32), ctx.empty((n, hw, c))
            ctx.check(ctx.lib.rcgan_act_meanhw_fwd(ctx.h, n, hw, c, xd.dtype, act, _p(xd), _p(feat)))
            ctx.check(ctx.lib.rcgan_act_meanhw_bwd(ctx.h, n, hw, c, xd.dtype, act, _p(xd), _p(dfd), _p(dx)))
            ref, mag = R.act_meanhw_fwd(x, act)
            B.close(what + " feat", feat, ref, R.sum_bound(hw, mag))
            dref = R.act_meanhw_bwd(x, dfeat, act)
            if mode == "f32":
                B.close(what + " dx", dx, dref, R.elem_bound(dref))
            else:
                B.half(what + " dx", dx, dref, mode)
            if (hw, c, act) == (49, 130, L.ACT_LRELU):
                feat2, dx2 = ctx.empty((n, c), L.F32), ctx.empty((n, hw, c))
                ctx.check(ctx.lib.rcgan_act_meanhw_fwd(ctx.h, n, hw, c, xd.dtype, act, _p(xd), _p(feat2)))
                ctx.check(ctx.lib.rcgan_act_meanhw_bwd(ctx.h, n, hw, c, xd.dtype, act, _p(xd), _p(dfd), _p(dx2)))
                B.same(what + " feat again", feat2, feat)
                B.same(what + " dx again", dx2, dx)
    B.done()


def test_act_meanhw_bwd_past_the_grid_cap(dev):
    """n * hw * c = 1 198 080 elements > 4096 blocks x 256 threads: the grid-stride loop takes a second round."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    n, hw, c = 9, 256, 520
    assert n * hw * c > 4096 * 256
    B = Batch(ctx)
    rs = np.random.RandomState(7)
    x = half_round(mode, _with_zeros(rs, (n, hw, c)))
    dfeat = rs.randn(n, c).astype(np.float32)
    xd, dfd, dx = ctx.upload(x), ctx.upload(dfeat, L.F32), ctx.empty((n, hw, c))
    ctx.check(ctx.lib.rcgan_act_meanhw_bwd(ctx.h, n, hw, c, xd.dtype, L.ACT_LRELU, _p(xd), _p(dfd), _p(dx)))
    dref = R.act_meanhw_bwd(x, dfeat, L.ACT_LRELU)
    if mode == "f32":
        B.close("act_meanhw_bwd past the cap", dx, dref, R.elem_bound(dref))
    else:
        B.half("act_meanhw_bwd past the cap", dx, dref, mode)
    B.done()


# ---------------------------------------------------------------------------------------------------- gather / scatter-add
def _index_sets(rs, n, v):
    perm = rs.permutation(v)[:n] if n <= v else rs.permutation(np.arange(n) % v)
    return {"all equal": np.full(n, rs.randint(v)), "permutation": perm, "random, rows absent": rs.randint(max(1, v // 2), size=n)}


def _scatter_case(B, ctx, what, src, idx, v, acc, rs):
    from rcgan_amd import _lib as L
    n, d = src.shape
    prev = rs.randn(v, d).astype(np.float32) if acc else None
    tg = ctx.upload(prev, L.F32) if acc else ctx.empty((v, d), L.F32)
    ctx.check(ctx.lib.rcgan_scatter_add_rows(ctx.h, n, d, v, _p(ctx.upload(src, L.F32)), _p(ctx.upload(idx)), _p(tg), acc))
    ref, mag = R.scatter_add_rows(src, idx, v, prev)
    cnt = np.bincount(idx, minlength=v)
    B.close(what, tg, ref, R.sum_bound((cnt + acc)[:, None], mag))
    absent = cnt == 0
    if acc:
        B.where(what + ": absent rows keep their bits", tg, lambda got: np.array_equal(_bits(got[absent]), _bits(prev[absent])))
    else:
        B.where(what + ": absent rows are exactly 0", tg, lambda got: (got[absent] == 0).all())
    return tg


@pytest.mark.parametrize("d", [1, 7, 128, 300])
def test_gather_and_scatter_add_rows(dev32, d):
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(200 + d)
    for v in (1, 10, 100, 1000):
        table = rs.randn(v, d).astype(np.float32)
        td = ctx.upload(table, L.F32)
        for n in (1, 6, 64):
            src = rs.randn(n, d).astype(np.float32)
            for name, idx in _index_sets(rs, n, v).items():
                idx = idx.astype(np.int32)
                what = "d %d v %d n %d %s" % (d, v, n, name)
                out = ctx.empty((n, d), L.F32)
                ctx.check(ctx.lib.rcgan_gather_rows(ctx.h, n, d, _p(td), _p(ctx.upload(idx)), _p(out)))
                B.bits("gather " + what, out, table[idx])
                for acc in (0, 1):
                    tg = _scatter_case(B, ctx, "scatter acc %d %s" % (acc, what), src, idx, v, acc, rs)
                if (v, n, name) == (100, 64, "random, rows absent"):
                    rs2 = np.random.RandomState(5)
                    a = _scatter_case(B, ctx, "scatter repeat a " + what, src, idx, v, 1, rs2)
                    rs2 = np.random.RandomState(5)
                    b = _scatter_case(B, ctx, "scatter repeat b " + what, src, idx, v, 1, rs2)
                    B.same("scatter again " + what, a, b)
                    out2 = ctx.empty((n, d), L.F32)
                    ctx.check(ctx.lib.rcgan_gather_rows(ctx.h, n, d, _p(td), _p(ctx.upload(idx)), _p(out2)))
                    B.same("gather again " + what, out2, out)
        B.done()


def test_gather_and_scatter_past_the_grid_cap(dev32):
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(9)
    n, d, v = 1100, 1000, 10
    assert n * d > 4096 * 256
    table, idx = rs.randn(v, d).astype(np.float32), rs.randint(v, size=n).astype(np.int32)
    out = ctx.empty((n, d), L.F32)
    ctx.check(ctx.lib.rcgan_gather_rows(ctx.h, n, d, _p(ctx.upload(table, L.F32)), _p(ctx.upload(idx)), _p(out)))
    B.bits("gather past the cap", out, table[idx])
    n, d, v = 8, 1100, 1024
    assert v * d > 4096 * 256
    src, idx = rs.randn(n, d).astype(np.float32), np.array([0, 1023, 1023, 500, 7, 7, 7, 931], np.int32)
    for acc in (0, 1):
        _scatter_case(B, ctx, "scatter past the cap acc %d" % acc, src, idx, v, acc, rs)
    B.done()


# ---------------------------------------------------------------------------------------------------- projection logit
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_proj_logit(dev32, n):
    """A wavefront per row, four rows per workgroup; psi NULL and not; every subset of the three gradients; acc_feat both ways."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(300 + n)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    for d in (1, 63, 64, 65, 128, 200):
        feat, emb, psi, g = (rs.randn(*s).astype(np.float32) for s in ((n, d), (n, d), (n,), (n,)))
        prev = rs.randn(n, d).astype(np.float32)
        fd, ed, pd, gd = up(feat), up(emb), up(psi), up(g)
        for with_psi in (False, True):
            what = "proj_logit n %d d %d psi %d" % (n, d, with_psi)
            lg = ctx.empty((n,), L.F32)
            ctx.check(ctx.lib.rcgan_proj_logit_fwd(ctx.h, n, d, _p(fd), _p(pd) if with_psi else None, _p(ed), _p(lg)))
            ref, mag = R.proj_logit_fwd(feat, psi if with_psi else None, emb)
            B.close(what, lg, ref, R.sum_bound(d + 1, mag))
            if d == 200:
                lg2 = ctx.empty((n,), L.F32)
                ctx.check(ctx.lib.rcgan_proj_logit_fwd(ctx.h, n, d, _p(fd), _p(pd) if with_psi else None, _p(ed), _p(lg2)))
                B.same(what + " again", lg2, lg)
        for wf, wp, we, acc in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            what = "proj_logit_bwd n %d d %d dfeat %d dpsi %d demb %d acc %d" % (n, d, wf, wp, we, acc)
            dfeat = up(prev) if (wf and acc) else ctx.empty((n, d), L.F32)
            dpsi, demb = ctx.empty((n,), L.F32), ctx.empty((n, d), L.F32)
            # (emb is read only for dfeat, feat only for demb: NULL where the header says it may be)
            ctx.check(ctx.lib.rcgan_proj_logit_bwd(ctx.h, n, d, _p(fd) if we else None, _p(ed) if wf else None, _p(gd), _p(dfeat) if wf else None,
                                                   _p(dpsi) if wp else None, _p(demb) if we else None, acc))
            rf, mf, rp, re = R.proj_logit_bwd(feat, emb, g, prev if acc else None)
            if wf:
                B.close(what + " dfeat", dfeat, rf, R.sum_bound(2, mf) if acc else R.elem_bound(rf))
            else:
                B.untouched(what + " dfeat", dfeat)
            B.bits(what + " dpsi", dpsi, rp) if wp else B.untouched(what + " dpsi", dpsi)
            B.close(what + " demb", demb, re, R.elem_bound(re)) if we else B.untouched(what + " demb", demb)
            if (d, wf, wp, we, acc) == (65, 1, 1, 1, 0):
                o = [ctx.empty((n, d), L.F32), ctx.empty((n,), L.F32), ctx.empty((n, d), L.F32)]
                ctx.check(ctx.lib.rcgan_proj_logit_bwd(ctx.h, n, d, _p(fd), _p(ed), _p(gd), _p(o[0]), _p(o[1]), _p(o[2]), 0))
                for a, b in zip(o, (dfeat, dpsi, demb)):
                    B.same(what + " again", a, b)
    B.done()


@pytest.mark.parametrize("v", [1, 10, 17, 100, 1000])
def test_proj_logit_all(dev32, v):
    """A wavefront per logit (n * v a multiple of 4 and not), a thread per output of the adjoint; zero rows in dlogits."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(400 + v)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    for n, d in itertools.product((1, 3, 6), (1, 65, 128)):
        feat, psi, E, dl = (rs.randn(*s).astype(np.float32) for s in ((n, d), (n,), (v, d), (n, v)))
        E *= 0.3
        if n > 1:
            dl[n // 2] = 0.0
        prev = rs.randn(n, d).astype(np.float32)
        fd, pd, Ed, dld = up(feat), up(psi), up(E), up(dl)
        what = "proj_logit_all n %d d %d v %d" % (n, d, v)
        lg = ctx.empty((n, v), L.F32)
        ctx.check(ctx.lib.rcgan_proj_logit_all_fwd(ctx.h, n, d, v, _p(fd), _p(pd), _p(Ed), _p(lg)))
        ref, mag = R.proj_logit_all_fwd(feat, psi, E)
        B.close(what, lg, ref, R.sum_bound(d + 1, mag))
        if (n, d) == (3, 65):
            lg2 = ctx.empty((n, v), L.F32)
            ctx.check(ctx.lib.rcgan_proj_logit_all_fwd(ctx.h, n, d, v, _p(fd), _p(pd), _p(Ed), _p(lg2)))
            B.same(what + " again", lg2, lg)
        outs = {}
        for acc in (0, 1, 0):
            dfeat = up(prev) if acc else ctx.empty((n, d), L.F32)
            dpsi, dE = ctx.empty((n,), L.F32), ctx.empty((v, d), L.F32)
            ctx.check(ctx.lib.rcgan_proj_logit_all_bwd(ctx.h, n, d, v, _p(fd), _p(Ed), _p(dld), _p(dfeat), _p(dpsi), _p(dE), acc))
            if acc == 0 and outs:                    # the second run of acc = 0: same bits
                for a, b in zip((dfeat, dpsi, dE), outs[0]):
                    B.same(what + " bwd again", a, b)
                continue
            outs[acc] = (dfeat, dpsi, dE)
            (rf, mf), (rp, mp), (rE, mE) = R.proj_logit_all_bwd(feat, E, dl, prev if acc else None)
            B.close(what + " dfeat acc %d" % acc, dfeat, rf, R.sum_bound(v + acc, mf))
            B.close(what + " dpsi acc %d" % acc, dpsi, rp, R.sum_bound(v, mp))
            B.close(what + " dE acc %d" % acc, dE, rE, R.sum_bound(n, mE))
            if n > 1 and not acc:
                B.where(what + ": a zero dlogits row gives exact zeros", dfeat, lambda got, r=n // 2: (got[r] == 0).all())
        if d == 128:
            B.done()
    B.done()


# ---------------------------------------------------------------------------------------------------- loss terms
LOSS_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (3, 100), (64, 100), (37, 1000)]
# (dwts non-NULL, dlogit non-NULL, loss_acc: None NULL / a value to add to, weight): every combination, dealt out over the cases in turn
LOSS_OPTIONS = list(itertools.product((0, 1), (0, 1), (None, 0.0, 3.25), (1.0, 0.5, -2.0)))


def _loss_inputs(rs, kind, rows, cols):
    """Hinge: some logits exactly +-1 (term and derivative 0).  Cross-entropy: [-80, 80] with +-{10, 12, 17, 30, 80} planted."""
    total = rows * cols
    if kind in (R.HINGE_REAL, R.HINGE_FAKE):
        x = rs.randn(total) * 2
        x[::3] = 1.0
        x[1::5] = -1.0
    elif kind == R.NEG_MEAN:
        x = rs.randn(total) * 3
    else:
        x = rs.uniform(-80, 80, size=total)
        plant = np.array([s * m for m in SAT for s in (1.0, -1.0)])
        k = min(total, plant.size)
        x[rs.permutation(total)[:k]] = plant[rs.permutation(plant.size)[:k]] if total < plant.size else plant
    return x.reshape(rows, cols).astype(np.float32)


@pytest.mark.parametrize("kind", [R.HINGE_REAL, R.HINGE_FAKE, R.NEG_MEAN, R.CE_ONES, R.CE_ZEROS])
def test_loss_fwd_bwd(dev32, kind):
    """One workgroup of 256 threads over rows x cols around 256 and far past it; weights, dwts, dlogit, loss_acc present and NULL."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(500 + kind)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    turn = itertools.cycle(LOSS_OPTIONS[kind::5] + LOSS_OPTIONS)
    for rows, cols in LOSS_SHAPES:
        x = _loss_inputs(rs, kind, rows, cols)
        if kind in (R.CE_ONES, R.CE_ZEROS) and rows * cols >= 10:
            assert all((x == s).any() and (x == -s).any() for s in SAT)
        wts = rs.randn(rows, cols).astype(np.float32)                # (C^-1 rows have negative entries)
        xd, wd = up(x), up(wts)
        for weighted in (0, 1):
            for _ in range(4):
                want_dw, want_dx, acc0, weight = next(turn)
                what = "loss kind %d %dx%d wts %d dwts %d dlogit %d loss_acc %s weight %g" % (kind, rows, cols, weighted, want_dw, want_dx, acc0, weight)
                dx, dw = ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32)
                loss = up([acc0]) if acc0 is not None else ctx.empty((1,), L.F32)
                ctx.check(ctx.lib.rcgan_loss_fwd_bwd(ctx.h, kind, rows, cols, _p(xd), _p(wd) if weighted else None, weight,
                                                     _p(loss) if acc0 is not None else None, _p(dx) if want_dx else None, _p(dw) if want_dw else None))
                val, mag, rdx, rdw = R.loss_fwd_bwd(kind, x, wts if weighted else None, weight)
                if acc0 is not None:
                    B.close(what + " loss", loss, np.array([acc0 + val]), R.sum_bound(rows * cols + 1, abs(acc0) + mag))
                else:
                    B.untouched(what + " loss", loss)
                B.close(what + " dlogit", dx, rdx, R.elem_bound(rdx)) if want_dx else B.untouched(what + " dlogit", dx)
                B.close(what + " dwts", dw, rdw, R.elem_bound(rdw)) if want_dw else B.untouched(what + " dwts", dw)
        if (rows, cols) == (64, 100):
            o = [[ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32), up([1.5])] for _ in range(2)]
            for dx, dw, loss in o:
                ctx.check(ctx.lib.rcgan_loss_fwd_bwd(ctx.h, kind, rows, cols, _p(xd), _p(wd), -2.0, _p(loss), _p(dx), _p(dw)))
            for a, b in zip(*o):
                B.same("loss kind %d again" % kind, a, b)
        B.done()


def _bce_inputs(rs, rows, cols):
    x = rs.uniform(-80, 80, size=(rows, cols)).astype(np.float32)
    lab = rs.randint(cols, size=rows).astype(np.int32)
    plant = np.array([s * m for m in SAT for s in (1.0, -1.0)], np.float32)
    x[np.arange(rows), lab] = plant[np.arange(rows) % plant.size]            # the labelled column is among the saturated ones
    if cols > 1:
        x[np.arange(rows), (lab + 1) % cols] = -plant[np.arange(rows) % plant.size]
    return x, lab


BCE_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (3, 100), (30, 10), (64, 100), (640, 10), (37, 1000)]


def test_bce_onehot_fwd_bwd(dev32):
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(600)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    turn = itertools.cycle(itertools.product((1, 0), (3.25, None, 0.0), (1.0, 0.5, -2.0)))
    for rows, cols in BCE_SHAPES:
        x, lab = _bce_inputs(rs, rows, cols)
        xd, ld = up(x), ctx.upload(lab)
        for _ in range(4):
            want_dx, acc0, weight = next(turn)
            what = "bce %dx%d dx %d loss_acc %s weight %g" % (rows, cols, want_dx, acc0, weight)
            dx = ctx.empty((rows, cols), L.F32)
            loss = up([acc0]) if acc0 is not None else ctx.empty((1,), L.F32)
            ctx.check(ctx.lib.rcgan_bce_onehot_fwd_bwd(ctx.h, rows, cols, _p(xd), _p(ld), weight, _p(loss) if acc0 is not None else None,
                                                       _p(dx) if want_dx else None))
            val, mag, rdx = R.bce_onehot_fwd_bwd(x, lab, weight)
            if acc0 is not None:
                B.close(what + " loss", loss, np.array([acc0 + val]), R.sum_bound(rows * cols + 1, abs(acc0) + mag))
            else:
                B.untouched(what + " loss", loss)
            B.close(what + " dx", dx, rdx, R.elem_bound(rdx)) if want_dx else B.untouched(what + " dx", dx)
        if (rows, cols) == (640, 10):
            o = [[ctx.empty((rows, cols), L.F32), up([1.5])] for _ in range(2)]
            for dx, loss in o:
                ctx.check(ctx.lib.rcgan_bce_onehot_fwd_bwd(ctx.h, rows, cols, _p(xd), _p(ld), 0.5, _p(loss), _p(dx)))
            for a, b in zip(*o):
                B.same("bce again", a, b)
    B.done()


def test_gradient_scale(dev32):
    """rcgan_set_grad_scale(1024, device 0.5): every gradient of the loss kernels is 512 x its unscaled bits, the loss values keep theirs."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(700)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    rows, cols = 3, 100
    half = up([0.5])
    wts = (rs.rand(rows, cols) + 0.5).astype(np.float32)         # (with |x| <= 80 every gradient stays a normal fp32 number: x 512 is exact)
    wd = up(wts)
    xb, lab = _bce_inputs(rs, rows, cols)
    xbd, ld = up(xb), ctx.upload(lab)
    runs = {}
    try:
        for scaled in (0, 1):
            ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1024.0 if scaled else 1.0, _p(half) if scaled else None))
            for kind in range(5):
                x = _loss_inputs(np.random.RandomState(kind), kind, rows, cols)
                dx, dw, loss = ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32), up([0.0])
                ctx.check(ctx.lib.rcgan_loss_fwd_bwd(ctx.h, kind, rows, cols, _p(up(x)), _p(wd), 1.0, _p(loss), _p(dx), _p(dw)))
                runs[(kind, scaled)] = (dx, dw, loss)
                if scaled:
                    val, mag, rdx, rdw = R.loss_fwd_bwd(kind, x, wts, 1.0, scale=512.0)
                    B.close("scaled dlogit kind %d" % kind, dx, rdx, R.elem_bound(rdx))
                    B.close("scaled dwts kind %d" % kind, dw, rdw, R.elem_bound(rdw))
                    B.close("loss under a gradient scale, kind %d" % kind, loss, np.array([val]), R.sum_bound(rows * cols + 1, mag))
            dx, loss = ctx.empty((rows, cols), L.F32), up([0.0])
            ctx.check(ctx.lib.rcgan_bce_onehot_fwd_bwd(ctx.h, rows, cols, _p(xbd), _p(ld), 1.0, _p(loss), _p(dx)))
            runs[("bce", scaled)] = (dx, loss)
            if scaled:
                val, mag, rdx = R.bce_onehot_fwd_bwd(xb, lab, 1.0, scale=512.0)
                B.close("scaled bce dx", dx, rdx, R.elem_bound(rdx))
    finally:
        ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1.0, None))
    for key in [k for k in runs if k[1] == 1]:
        plain, scaled = runs[(key[0], 0)], runs[key]
        for a, b in zip(plain[:-1], scaled[:-1]):
            B.where("gradient of %s: 512 x the unscaled bits" % (key[0],), b, lambda got, a=a: np.array_equal(_bits(got), _bits(512.0 * ctx.download(a))))
        B.same("loss value of %s unchanged by the scale" % (key[0],), scaled[-1], plain[-1])
    B.done()


# ---------------------------------------------------------------------------------------------------- softmax rows
def _softmax_rows_input(rs, rows, cols):
    l = rs.randn(rows, cols) * 2
    for r in range(rows):
        k = r % 4
        if k == 0:
            l[r] = 2.5                                           # constant
        elif k == 1:
            l[r] = rs.uniform(-80, 80, size=cols)                # spread +-80
            l[r, 0] = 80.0
            l[r, -1] = -80.0 if cols > 1 else 80.0
        elif k == 2:
            l[r] += 1e4                                          # overflows without the max subtraction
        else:
            l[r, rs.randint(cols)] += 50.0                       # one dominant entry
    return l.astype(np.float32)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 100])
def test_softmax_rows(dev32, rows):
    """A thread per row, 64 per block."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    rs = np.random.RandomState(800 + rows)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    for cols in (1, 2, 10, 100, 1000):
        what = "softmax %dx%d" % (rows, cols)
        l = _softmax_rows_input(rs, rows, cols)
        ld, p = up(l), ctx.empty((rows, cols), L.F32)
        ctx.check(ctx.lib.rcgan_softmax_rows_fwd(ctx.h, rows, cols, _p(ld), _p(p)))
        ref, bound = R.softmax_rows_fwd(l)
        B.close(what, p, ref, bound)
        B.where(what + ": rows sum to 1 within cols * 2^-24", p, lambda got, c=cols: (np.abs(got.astype(np.float64).sum(1) - 1.0) <= c * EPS32).all())
        p32 = ref.astype(np.float32)
        dp, prev = rs.randn(rows, cols).astype(np.float32), rs.randn(rows, cols).astype(np.float32)
        pd, dpd = up(p32), up(dp)
        outs = []
        for acc in (0, 1, 0):
            dl = up(prev) if acc else ctx.empty((rows, cols), L.F32)
            ctx.check(ctx.lib.rcgan_softmax_rows_bwd(ctx.h, rows, cols, _p(pd), _p(dpd), _p(dl), acc))
            new = R.softmax_rows_bwd(p32, dp)
            if acc:
                B.close(what + " bwd acc 1", dl, new + prev, _added(new, prev))
            elif not outs:
                B.close(what + " bwd acc 0", dl, new, R.elem_bound(new))
                outs.append(dl)
            else:
                B.same(what + " bwd again", dl, outs[0])
        if cols == 10:
            p2 = ctx.empty((rows, cols), L.F32)
            ctx.check(ctx.lib.rcgan_softmax_rows_fwd(ctx.h, rows, cols, _p(ld), _p(p2)))
            B.same(what + " again", p2, p)
    B.done()


# ---------------------------------------------------------------------------------------------------- inference batch norm
@pytest.mark.parametrize("c", [1, 10, 64, 130])
def test_bn_infer_and_its_adjoint(dev, c):
    """rows * c a multiple of the 256-thread block (rows = 256) and not (rows = 3); moving_var with zeros: eps alone in the root."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    B = Batch(ctx)
    rs = np.random.RandomState(900 + c)
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    eps = float(np.float32(1e-5))                    # (the value that crosses the ABI)
    gamma, beta, mm, mv = ((rs.rand(c) + 0.5).astype(np.float32), rs.randn(c).astype(np.float32), rs.randn(c).astype(np.float32),
                           rs.rand(c).astype(np.float32))
    mv[::3] = 0.0
    gd, bd, mmd, mvd = up(gamma), up(beta), up(mm), up(mv)
    for rows in (3, 256):
        assert (rows * c % 256 == 0) == (rows == 256)
        x = half_round(mode, rs.randn(rows, c) * 0.05 + mm)           # (1 / sqrt(eps) = 316: keep the normalised values moderate)
        dy, prev = half_round(mode, rs.randn(rows, c)), half_round(mode, rs.randn(rows, c))
        xd, dyd = ctx.upload(x), ctx.upload(dy)
        for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SIGMOID):
            what = "bn_infer %dx%d act %d %s" % (rows, c, act, mode)
            y = ctx.empty((rows, c))
            ctx.check(ctx.lib.rcgan_bn_infer(ctx.h, rows, c, xd.dtype, _p(xd), _p(gd), _p(bd), _p(mmd), _p(mvd), eps, act, _p(y)))
            ref, pre = R.bn_infer(x, gamma, beta, mm, mv, eps, act)
            if mode == "f32":
                # the pre-activation value is a two-term sum (scaled x + beta); the activation is 1-Lipschitz and elementwise
                B.close(what, y, ref, R.sum_bound(2, np.abs(pre - beta) + np.abs(beta)) + R.elem_bound(ref))
            else:
                B.half(what, y, ref, mode)
            if (rows, act) == (256, L.ACT_SIGMOID):
                y2 = ctx.empty((rows, c))
                ctx.check(ctx.lib.rcgan_bn_infer(ctx.h, rows, c, xd.dtype, _p(xd), _p(gd), _p(bd), _p(mmd), _p(mvd), eps, act, _p(y2)))
                B.same(what + " again", y2, y)
            yin = half_round(mode, ref)
            yin.reshape(-1)[::5] = 0.0 if act in (L.ACT_RELU, L.ACT_LRELU) else yin.reshape(-1)[::5]       # exact zeros: the negative side
            yd = ctx.upload(yin)
            outs = []
            for acc in (0, 1, 0):
                dx = ctx.upload(prev) if acc else ctx.empty((rows, c))
                ctx.check(ctx.lib.rcgan_bn_infer_bwd(ctx.h, rows, c, xd.dtype, _p(yd), _p(dyd), _p(gd), _p(mvd), eps, act, _p(dx), acc))
                new = R.bn_infer_bwd(yin, dy, gamma, mv, eps, act)
                if acc == 0 and outs:
                    if (rows, act) == (256, L.ACT_TANH):
                        B.same(what + " bwd again", dx, outs[0])
                    continue
                outs.append(dx)
                if mode == "f32":
                    B.close(what + " bwd acc %d" % acc, dx, new + prev if acc else new, _added(new, prev) if acc else R.elem_bound(new))
                else:
                    B.half(what + " bwd acc %d" % acc, dx, new + prev if acc else new, mode)
    B.done()


# ---------------------------------------------------------------------------------------------------- the fused head on saturated logits
@pytest.mark.parametrize("v", [10, 17])
@pytest.mark.parametrize("kind", [R.CE_ONES, R.CE_ZEROS])
def test_fused_head_saturated_logits(dev32, v, kind):
    """rcgan_proj_head_fwd_bwd, both routes (v = 10: label embeddings in LDS; v = 17: the wide route), every logit in [12, 30] under CE_ONES
    and in [-30, -12] under CE_ZEROS, a one-hot part and a weight-row part: dfeat and the five parameter gradients against float64 at
    1e-4 of max|ref|.  The subtracted form of the sigmoid gradient misses this by one to two orders of magnitude."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    B = Batch(ctx)
    n, d, ed, rows_a, weight = 6, 128, 300, 3, 2.0
    sign = 1.0 if kind == R.CE_ONES else -1.0
    rs = np.random.RandomState(v * 10 + kind)
    t = np.linspace(0.05, 1.0, n)
    feat = (rs.rand(n, d) * t[:, None]).astype(np.float32)
    s_out, s_e = np.float32(1.3), np.float32(0.7)
    w_out = np.full((d,), sign * 12.0 / (0.5 * d) * float(s_out), np.float32)       # psi = +-(14 + 12 t): 14.6 .. 26.6, E adds < 1
    b_out = np.array([sign * 14.0], np.float32)
    table = (rs.randn(v, ed) * 0.05).astype(np.float32)
    w_e = (rs.randn(ed, d) * 0.05).astype(np.float32)
    b_e = (rs.randn(d) * 0.01).astype(np.float32)
    lab = rs.randint(v, size=rows_a).astype(np.int32)
    wts = rs.rand(n - rows_a, v).astype(np.float32)
    f64 = R.f64
    E = f64(table) @ f64(w_e) / float(s_e) + f64(b_e)
    psi = f64(feat) @ f64(w_out) / float(s_out) + float(b_out[0])
    lg = psi[:, None] + f64(feat) @ E.T
    assert (sign * lg >= 12).all() and (sign * lg <= 30).all(), (lg.min(), lg.max())
    W = np.concatenate([np.eye(v)[lab] / rows_a, f64(wts) / (n - rows_a)])
    _, dterm = R.loss_term(kind, lg)
    dlg = weight * dterm * W
    dpsi = dlg.sum(1)
    dE = dlg.T @ f64(feat)
    ref = dict(dfeat=dlg @ E + dpsi[:, None] * f64(w_out) / float(s_out), dw_out=f64(feat).T @ dpsi, db_out=np.array([dpsi.sum()]),
               dtable=dE @ f64(w_e).T / float(s_e), dw_e=f64(table).T @ dE, db_e=dE.sum(0))
    up = lambda a: ctx.upload(np.asarray(a, np.float32), L.F32)
    hd = L.HeadDesc(n, d, v, ed, rows_a, kind, kind, weight)
    labd, wd = ctx.upload(lab), up(wts)
    hd.labels_a, hd.wts_b = labd.ptr, wd.ptr
    out = dict(dfeat=ctx.empty((n, d), L.F32), dw_out=up(np.zeros(d)), db_out=up(np.zeros(1)), dtable=up(np.zeros((v, ed))),
               dw_e=up(np.zeros((ed, d))), db_e=up(np.zeros(d)))
    loss, logits = up([0.0]), ctx.empty((n, v), L.F32)
    ctx.check(ctx.lib.rcgan_proj_head_fwd_bwd(
        ctx.h, C.byref(hd), _p(up(feat)), _p(up(w_out)), _p(up([s_out])), _p(up(b_out)), _p(up(table)), _p(up(w_e)), _p(up([s_e])), _p(up(b_e)),
        _p(loss), _p(logits), _p(out["dfeat"]), _p(out["dw_out"]), _p(out["db_out"]), _p(out["dtable"]), _p(out["dw_e"]), _p(out["db_e"]),
        C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
    ctx.check(ctx.lib.rcgan_head_flush(ctx.h))
    for k, t_ in out.items():
        B.where("fused head v %d kind %d %s" % (v, kind, k), t_,
                lambda got, k=k: (assert_close(got.reshape(ref[k].shape), ref[k], 1e-4, "fused head %s" % k), True)[1])
    B.where("fused head logits written", logits, lambda got: np.isfinite(got).all())
    B.done()


# ---------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_on_the_paths_the_one_shape_test_leaves_out(dev32):
    """ops.proj_logit_all whose psi already carries a gradient (scratch + axpby), ops.gather_rows backward onto a table.grad that holds
    values (scatter-add with accumulate), ops.loss_term on a 1-D input of 257 rows."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    from tests.gpu_util import FakeParam
    ctx, _ = dev32
    g = ctx.guard
    g.clear()
    rs = np.random.RandomState(11)
    n, d, v = 5, 65, 17
    feat, psi, E = FakeParam(ctx, rs.randn(n, d)), FakeParam(ctx, rs.randn(n)), FakeParam(ctx, rs.randn(v, d) * 0.3)
    E.t.grad = None
    g0 = rs.randn(n).astype(np.float32)
    ctx.upload(g0, L.F32, out=psi.t.grad)
    lg = O.proj_logit_all(ctx, feat.t, psi.t, E.t)
    dl = rs.randn(n, v).astype(np.float32)
    lg.grad = ctx.upload(dl, L.F32)
    ctx.backward()
    ctx.sync()
    g.check()
    F_, E_ = (ctx.download(p.t) for p in (feat, E))
    (rf, mf), (rp, mp), (rE, mE) = R.proj_logit_all_bwd(F_, E_, dl)
    assert R.worst(psi.grad(ctx), rp + g0, R.sum_bound(v + 1, mp + np.abs(g0))) <= 1.0
    assert R.worst(feat.grad(ctx), rf, R.sum_bound(v + 1, mf)) <= 1.0                 # (FakeParam gradients start at 0: accumulate)
    assert R.worst(ctx.download(E.t.grad), rE, R.sum_bound(n, mE)) <= 1.0

    ctx.new_step()
    vv, dd, nn_ = 10, 7, 6
    table = FakeParam(ctx, rs.randn(vv, dd))
    prev = rs.randn(vv, dd).astype(np.float32)
    ctx.upload(prev, L.F32, out=table.t.grad)
    idx = np.array([3, 3, 9, 0, 3, 9], np.int32)
    e = O.gather_rows(ctx, table.t, ctx.upload(idx), nn_)
    assert np.array_equal(_bits(ctx.download(e)), _bits(ctx.download(table.t)[idx]))
    src = rs.randn(nn_, dd).astype(np.float32)
    e.grad = ctx.upload(src, L.F32)
    ctx.backward()
    ctx.sync()
    g.check()
    ref, mag = R.scatter_add_rows(src, idx, vv, prev)
    got = table.grad(ctx)
    cnt = np.bincount(idx, minlength=vv)
    assert R.worst(got, ref, R.sum_bound((cnt + 1)[:, None], mag)) <= 1.0
    assert np.array_equal(_bits(got[cnt == 0]), _bits(prev[cnt == 0]))

    ctx.new_step()
    x = _loss_inputs(rs, R.CE_ONES, 257, 1).reshape(-1)
    xp = FakeParam(ctx, x)
    xp.t.grad = None
    loss = ctx.persistent((1,), L.F32, fill=0.0)
    O.loss_term(ctx, L.LOSS_CE_ONES, xp.t, 0.5, loss)
    ctx.sync()
    g.check()
    val, mag, rdx, _ = R.loss_fwd_bwd(R.CE_ONES, x, None, 0.5)
    assert g.unwritten(xp.t.grad) == 0
    assert R.worst(ctx.download(loss), np.array([val]), R.sum_bound(258, mag)) <= 1.0
    assert R.worst(ctx.download(xp.t.grad), rdx.reshape(-1), R.elem_bound(rdx.reshape(-1))) <= 1.0
    ctx.new_step()


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_anything_is_launched(dev32):
    """A non-positive dimension or a NULL required tensor: RCGAN_EINVALID_ARG with a message, every buffer still all fill, bands clean.
    (Only arguments the entry points' own checks refuse: nothing here may reach a kernel.)"""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    g = ctx.guard
    g.clear()
    lib, h = ctx.lib, ctx.h
    bufs = [ctx.empty((64,), L.F32) for _ in range(7)]
    a, b, c_, d_, e, f, o = (_p(t) for t in bufs)
    ib = ctx.empty((64,), "i32")
    i = _p(ib)
    N = None
    F32 = L.F32
    calls = {
        "act_meanhw_fwd n 0": lambda: lib.rcgan_act_meanhw_fwd(h, 0, 2, 2, F32, 0, a, o),
        "act_meanhw_fwd hw 0": lambda: lib.rcgan_act_meanhw_fwd(h, 2, 0, 2, F32, 0, a, o),
        "act_meanhw_fwd c -1": lambda: lib.rcgan_act_meanhw_fwd(h, 2, 2, -1, F32, 0, a, o),
        "act_meanhw_fwd x NULL": lambda: lib.rcgan_act_meanhw_fwd(h, 2, 2, 2, F32, 0, N, o),
        "act_meanhw_fwd feat NULL": lambda: lib.rcgan_act_meanhw_fwd(h, 2, 2, 2, F32, 0, a, N),
        "act_meanhw_bwd hw 0": lambda: lib.rcgan_act_meanhw_bwd(h, 2, 0, 2, F32, 0, a, b, o),
        "act_meanhw_bwd dfeat NULL": lambda: lib.rcgan_act_meanhw_bwd(h, 2, 2, 2, F32, 0, a, N, o),
        "act_meanhw_bwd dx NULL": lambda: lib.rcgan_act_meanhw_bwd(h, 2, 2, 2, F32, 0, a, b, N),
        "gather_rows n 0": lambda: lib.rcgan_gather_rows(h, 0, 2, a, i, o),
        "gather_rows d 0": lambda: lib.rcgan_gather_rows(h, 2, 0, a, i, o),
        "gather_rows idx NULL": lambda: lib.rcgan_gather_rows(h, 2, 2, a, N, o),
        "gather_rows out NULL": lambda: lib.rcgan_gather_rows(h, 2, 2, a, i, N),
        "scatter_add_rows v 0": lambda: lib.rcgan_scatter_add_rows(h, 2, 2, 0, a, i, o, 0),
        "scatter_add_rows n -3": lambda: lib.rcgan_scatter_add_rows(h, -3, 2, 2, a, i, o, 0),
        "scatter_add_rows src NULL": lambda: lib.rcgan_scatter_add_rows(h, 2, 2, 2, N, i, o, 0),
        "scatter_add_rows table_grad NULL": lambda: lib.rcgan_scatter_add_rows(h, 2, 2, 2, a, i, N, 1),
        "proj_logit_fwd d 0": lambda: lib.rcgan_proj_logit_fwd(h, 2, 0, a, b, c_, o),
        "proj_logit_fwd emb NULL": lambda: lib.rcgan_proj_logit_fwd(h, 2, 2, a, b, N, o),
        "proj_logit_fwd logit NULL": lambda: lib.rcgan_proj_logit_fwd(h, 2, 2, a, b, c_, N),
        "proj_logit_bwd n 0": lambda: lib.rcgan_proj_logit_bwd(h, 0, 2, a, b, c_, d_, e, o, 0),
        "proj_logit_bwd dlogit NULL": lambda: lib.rcgan_proj_logit_bwd(h, 2, 2, a, b, N, d_, e, o, 0),
        "proj_logit_bwd dfeat without emb": lambda: lib.rcgan_proj_logit_bwd(h, 2, 2, a, N, c_, o, N, N, 0),
        "proj_logit_bwd demb without feat": lambda: lib.rcgan_proj_logit_bwd(h, 2, 2, N, b, c_, N, N, o, 0),
        "proj_logit_all_fwd v 0": lambda: lib.rcgan_proj_logit_all_fwd(h, 2, 2, 0, a, b, c_, o),
        "proj_logit_all_fwd psi NULL": lambda: lib.rcgan_proj_logit_all_fwd(h, 2, 2, 2, a, N, c_, o),
        "proj_logit_all_fwd logits NULL": lambda: lib.rcgan_proj_logit_all_fwd(h, 2, 2, 2, a, b, c_, N),
        "proj_logit_all_bwd d 0": lambda: lib.rcgan_proj_logit_all_bwd(h, 2, 0, 2, a, b, c_, d_, e, o, 0),
        "proj_logit_all_bwd dfeat NULL": lambda: lib.rcgan_proj_logit_all_bwd(h, 2, 2, 2, a, b, c_, N, e, o, 0),
        "proj_logit_all_bwd dpsi NULL": lambda: lib.rcgan_proj_logit_all_bwd(h, 2, 2, 2, a, b, c_, d_, N, o, 0),
        "proj_logit_all_bwd dE NULL": lambda: lib.rcgan_proj_logit_all_bwd(h, 2, 2, 2, a, b, c_, d_, o, N, 0),
        "loss_fwd_bwd kind 5": lambda: lib.rcgan_loss_fwd_bwd(h, 5, 2, 2, a, N, 1.0, b, o, N),
        "loss_fwd_bwd rows 0": lambda: lib.rcgan_loss_fwd_bwd(h, 0, 0, 2, a, N, 1.0, b, o, N),
        "loss_fwd_bwd cols -1": lambda: lib.rcgan_loss_fwd_bwd(h, 0, 2, -1, a, N, 1.0, b, o, N),
        "loss_fwd_bwd x NULL": lambda: lib.rcgan_loss_fwd_bwd(h, 0, 2, 2, N, N, 1.0, b, o, N),
        "bce_onehot rows 0": lambda: lib.rcgan_bce_onehot_fwd_bwd(h, 0, 2, a, i, 1.0, b, o),
        "bce_onehot x NULL": lambda: lib.rcgan_bce_onehot_fwd_bwd(h, 2, 2, N, i, 1.0, b, o),
        "bce_onehot labels NULL": lambda: lib.rcgan_bce_onehot_fwd_bwd(h, 2, 2, a, N, 1.0, b, o),
        "softmax_rows_fwd cols 0": lambda: lib.rcgan_softmax_rows_fwd(h, 2, 0, a, o),
        "softmax_rows_fwd logits NULL": lambda: lib.rcgan_softmax_rows_fwd(h, 2, 2, N, o),
        "softmax_rows_fwd p NULL": lambda: lib.rcgan_softmax_rows_fwd(h, 2, 2, a, N),
        "softmax_rows_bwd rows 0": lambda: lib.rcgan_softmax_rows_bwd(h, 0, 2, a, b, o, 0),
        "softmax_rows_bwd dp NULL": lambda: lib.rcgan_softmax_rows_bwd(h, 2, 2, a, N, o, 0),
        "softmax_rows_bwd dlogits NULL": lambda: lib.rcgan_softmax_rows_bwd(h, 2, 2, a, b, N, 1),
        "bn_infer rows 0": lambda: lib.rcgan_bn_infer(h, 0, 2, F32, a, b, c_, d_, e, 1e-5, 0, o),
        "bn_infer c 0": lambda: lib.rcgan_bn_infer(h, 2, 0, F32, a, b, c_, d_, e, 1e-5, 0, o),
        "bn_infer moving_var NULL": lambda: lib.rcgan_bn_infer(h, 2, 2, F32, a, b, c_, d_, N, 1e-5, 0, o),
        "bn_infer y NULL": lambda: lib.rcgan_bn_infer(h, 2, 2, F32, a, b, c_, d_, e, 1e-5, 0, N),
        "bn_infer_bwd rows 0": lambda: lib.rcgan_bn_infer_bwd(h, 0, 2, F32, a, b, c_, d_, 1e-5, 0, o, 0),
        "bn_infer_bwd act 9": lambda: lib.rcgan_bn_infer_bwd(h, 2, 2, F32, a, b, c_, d_, 1e-5, 9, o, 0),
        "bn_infer_bwd y NULL under ReLU": lambda: lib.rcgan_bn_infer_bwd(h, 2, 2, F32, N, b, c_, d_, 1e-5, L.ACT_RELU, o, 0),
        "bn_infer_bwd dy NULL": lambda: lib.rcgan_bn_infer_bwd(h, 2, 2, F32, a, N, c_, d_, 1e-5, 0, o, 0),
        "bn_infer_bwd dx NULL": lambda: lib.rcgan_bn_infer_bwd(h, 2, 2, F32, a, b, c_, d_, 1e-5, 0, N, 1),
    }
    for what, call in calls.items():
        assert call() == L.EINVALID_ARG, what
        assert len(lib.rcgan_last_error(h)) > 0, what
    ctx.sync()
    g.check()
    for t in bufs + [ib]:
        assert g.unwritten(t) == t.size, "a refused call wrote to a buffer"
    ctx.new_step()
