"""rcgan_pair_consistency_fwd_bwd (csrc/loss.hip) through the C ABI against the float64 restatement of its definition
(tests/bcr_ref.py), between guard bands (tests/guard.py: 0xFF margins around every buffer, fresh arena memory 0xFF-filled).

Shapes: pairs 1, 2, 63, 64, 65, 257 x cols 1, 10, 16, 17, 100 -- element counts on both sides of one pass of the 256 threads, multiples
of four (the 16-byte route) and not (the element route).  cols == 1 is a labelled part, without weights; every other case has weight
rows that sum to 1 and contain negative entries.  Bounds: tests/bcr_ref.bounds, from the number format alone -- per gradient element a
few fp32 ulps of 2 lam |w| |x - x_aug| / pairs plus the rounding of the accumulate add; for the value the forward error bound of an
fp32 sum of pairs * cols terms, gamma_n sum|t| (the bound tests/test_gpu_lecam_update.py uses for its sums)."""
import ctypes as C

import numpy as np
import pytest

from tests import bcr_ref as BR
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

PAIRS = (1, 2, 63, 64, 65, 257)
COLS = (1, 10, 16, 17, 100)
_env = {}


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    if _env:
        _env["cm"].__exit__(None, None, None)
        _env["ctx"].close()
        _env.clear()


def env():
    if not _env:
        ctx = make_ctx("f32", arena=1 << 20)          # (its own arena is replaced by the guarded one)
        cm = guarded(ctx, arena_bytes=64 << 20, ws_bytes=1 << 20)
        _env.update(ctx=ctx, cm=cm, g=cm.__enter__())
    _env["g"].clear()
    return _env["ctx"], _env["g"]


def _ptr(t, off=0):
    return C.c_void_p(t.ptr + off) if t is not None else None


def _weights(rs, rows, cols):
    """Rows that sum to 1 with negative entries among them (what C^-1 rows look like)."""
    w = rs.randn(rows, cols)
    w += (1.0 - w.sum(1, keepdims=True)) / cols
    assert (w < 0).any() or rows * cols < 4
    return w.astype(np.float32)


def _case(pairs, cols, seed=0):
    rs = np.random.RandomState(1000 * pairs + cols + seed)
    x = (rs.randn(pairs, cols) * 2 + 1.5).astype(np.float32)
    xa = (x + rs.randn(pairs, cols) * 0.5).astype(np.float32)
    w = _weights(rs, pairs, cols) if cols > 1 else None
    return rs, x, xa, w


def _up(ctx, a):
    from rcgan_amd import _lib as L
    return None if a is None else ctx.upload(np.ascontiguousarray(a, np.float32), dtype=L.F32)


def call(ctx, g, x, xa, w, lam, loss=None, term=None, dx=None, acc=0, dxa=None, dw=None, pairs=None, cols=None):
    p, c = (x.shape[0], x.shape[1] if len(x.shape) > 1 else 1)
    rc = ctx.lib.rcgan_pair_consistency_fwd_bwd(ctx.h, p if pairs is None else pairs, c if cols is None else cols, _ptr(x), _ptr(xa),
                                                _ptr(w), lam, _ptr(loss), _ptr(term), _ptr(dx), acc, _ptr(dxa), _ptr(dw))
    ctx.sync()
    g.check()
    return rc


def _check(ctx, x, xa, w, lam, outs, scale=1.0, dx_before=None, dw_before=None, what=""):
    loss, term, dx, dxa, dw = outs
    ref = BR.pair_consistency(x, xa, w, lam, scale)
    bd = BR.bounds(x, xa, w, lam, scale, dx_before=dx_before, dwts_before=dw_before)
    got_l, got_t = float(ctx.download(loss)[0]), float(ctx.download(term)[0])
    print("%s value %r want %r (bound %.3e); term %r want %r" % (what, got_l, ref["value"], bd["value"], got_t, ref["term"]))
    assert abs(got_l - ref["value"]) <= bd["value"], (what, got_l, ref["value"], bd["value"])
    assert abs(got_t - ref["term"]) <= bd["term"] + BR.ULP * abs(ref["term"]), (what, got_t, ref["term"], bd["term"])
    want_dx = ref["dx"] + (0 if dx_before is None else np.asarray(dx_before, np.float64).reshape(ref["dx"].shape))
    for name, t, want, b in (("dx", dx, want_dx, bd["dx"]), ("dx_aug", dxa, ref["dx_aug"], bd["dx_aug"])):
        err = np.abs(ctx.download(t).astype(np.float64).reshape(want.shape) - want)
        assert (err <= b).all(), (what, name, float((err - b).max()))
    if w is not None:
        want = ref["dwts"] + (0 if dw_before is None else np.asarray(dw_before, np.float64).reshape(ref["dwts"].shape))
        err = np.abs(ctx.download(dw).astype(np.float64).reshape(want.shape) - want)
        assert (err <= bd["dwts"]).all(), (what, "dwts", float((err - bd["dwts"]).max()))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("pairs", PAIRS)
def test_against_the_float64_reference(pairs, cols):
    """accumulate = 1 adds to a pre-filled dx and to a pre-filled dwts; dx_aug, pre-filled with 0xFF by the guarded arena, is
    overwritten in full; accumulate = 0 overwrites a 0xFF dx."""
    from rcgan_amd import _lib as L
    ctx, g = env()
    rs, x, xa, w = _case(pairs, cols)
    lam = 10.0
    dx0 = rs.randn(pairs, cols).astype(np.float32)
    dw0 = rs.randn(pairs, cols).astype(np.float32) if w is not None else None
    dev = [_up(ctx, a) for a in (x, xa, w)]
    # accumulate
    loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
    dx, dw, dxa = _up(ctx, dx0), _up(ctx, dw0), ctx.empty((pairs, cols), L.F32)
    assert g.unwritten(dxa) == pairs * cols
    assert call(ctx, g, *dev, lam, loss, term, dx, 1, dxa, dw, pairs, cols) == 0
    assert g.unwritten(dxa) == 0
    _check(ctx, x, xa, w, lam, (loss, term, dx, dxa, dw), dx_before=dx0, dw_before=dw0, what="%d x %d accumulate" % (pairs, cols))
    # overwrite
    loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
    dx, dxa, dw = ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32), _up(ctx, None if w is None else np.zeros((pairs, cols)))
    assert call(ctx, g, *dev, lam, loss, term, dx, 0, dxa, dw, pairs, cols) == 0
    assert g.unwritten(dx) == 0 and g.unwritten(dxa) == 0
    _check(ctx, x, xa, w, lam, (loss, term, dx, dxa, dw), what="%d x %d overwrite" % (pairs, cols))
    # a labelled part is x - x_aug alone: minus dx is dx_aug, bit for bit
    assert np.array_equal(ctx.download(dx), -ctx.download(dxa))


def test_the_element_route_on_buffers_off_the_16_byte_grid():
    """64 x 16 elements, every tensor 4 bytes past a 16-byte boundary: the element route -- against the reference, and within
    rounding of the 16-byte route's result on the same numbers."""
    from rcgan_amd import _lib as L
    ctx, g = env()
    pairs, cols, lam = 64, 16, 3.0
    rs, x, xa, w = _case(pairs, cols, seed=7)
    pad = lambda a: _up(ctx, np.concatenate([np.zeros(1, np.float32), a.reshape(-1)]))
    xs, xas, ws = pad(x), pad(xa), pad(w)
    loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
    n = pairs * cols
    dx, dxa, dw = _up(ctx, np.zeros(n + 1)), ctx.empty((n + 1,), L.F32), _up(ctx, np.zeros(n + 1))
    rc = ctx.lib.rcgan_pair_consistency_fwd_bwd(ctx.h, pairs, cols, _ptr(xs, 4), _ptr(xas, 4), _ptr(ws, 4), lam, _ptr(loss), _ptr(term),
                                                _ptr(dx, 4), 1, _ptr(dxa, 4), _ptr(dw, 4))
    assert rc == 0
    ctx.sync()
    g.check()
    assert g.unwritten(dxa) == 1 and ctx.download(dx)[0] == 0 and ctx.download(dw)[0] == 0          # (the element in front: untouched)
    ref, bd = BR.pair_consistency(x, xa, w, lam), BR.bounds(x, xa, w, lam, dx_before=np.zeros((pairs, cols)))
    assert abs(float(ctx.download(loss)[0]) - ref["value"]) <= bd["value"]
    assert (np.abs(ctx.download(dx)[1:].reshape(pairs, cols) - ref["dx"]) <= bd["dx"]).all()
    assert (np.abs(ctx.download(dxa)[1:].reshape(pairs, cols) - ref["dx_aug"]) <= bd["dx_aug"]).all()
    assert (np.abs(ctx.download(dw)[1:].reshape(pairs, cols) - ref["dwts"]) <= bd["dwts"]).all()


@pytest.mark.parametrize("pairs,cols", [(64, 1), (65, 10), (257, 16)])
def test_identical_halves_give_exactly_zero(pairs, cols):
    from rcgan_amd import _lib as L
    ctx, g = env()
    rs, x, _, w = _case(pairs, cols)
    dev = [_up(ctx, a) for a in (x, x.copy(), w)]
    loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
    dx, dxa, dw = ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32), _up(ctx, None if w is None else np.zeros((pairs, cols)))
    assert call(ctx, g, *dev, 10.0, loss, term, dx, 0, dxa, dw, pairs, cols) == 0
    assert ctx.download(loss)[0] == 0 and ctx.download(term)[0] == 0
    assert not ctx.download(dx).any() and not ctx.download(dxa).any() and (w is None or not ctx.download(dw).any())
    # ... and added to a gradient that is there already, they leave its bits
    dx0 = rs.randn(pairs, cols).astype(np.float32)
    dx = _up(ctx, dx0)
    assert call(ctx, g, *dev, 10.0, loss, term, dx, 1, dxa, dw, pairs, cols) == 0
    assert np.array_equal(ctx.download(dx).view(np.uint32), dx0.view(np.uint32))


def test_lam_zero_leaves_every_output_untouched():
    from rcgan_amd import _lib as L
    ctx, g = env()
    pairs, cols = 65, 10
    rs, x, xa, w = _case(pairs, cols)
    dev = [_up(ctx, a) for a in (x, xa, w)]
    outs = [ctx.empty((1,), L.F32), ctx.empty((1,), L.F32), ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32),
            ctx.empty((pairs, cols), L.F32)]
    for acc in (0, 1):
        assert call(ctx, g, *dev, 0.0, outs[0], outs[1], outs[2], acc, outs[3], outs[4], pairs, cols) == 0
        for t in outs:
            assert g.unwritten(t) == t.size


def test_the_gradient_scale_multiplies_the_gradients_exactly_and_leaves_the_loss_alone():
    from rcgan_amd import _lib as L
    ctx, g = env()
    pairs, cols, lam = 65, 10, 10.0
    rs, x, xa, w = _case(pairs, cols)
    dev = [_up(ctx, a) for a in (x, xa, w)]
    dev_scale = _up(ctx, np.array([32.0]))
    res = []
    try:
        for host, devp in ((1.0, None), (1024.0, None), (32.0, dev_scale)):
            ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, host, _ptr(devp)))
            loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
            dx, dxa, dw = ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32), _up(ctx, np.zeros((pairs, cols)))
            assert call(ctx, g, *dev, lam, loss, term, dx, 0, dxa, dw, pairs, cols) == 0
            res.append([ctx.download(t) for t in (loss, term, dx, dxa, dw)])
    finally:
        ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1.0, None))
    for scaled in res[1:]:
        assert np.array_equal(scaled[0], res[0][0]) and np.array_equal(scaled[1], res[0][1])
        for a, b in zip(res[0][2:], scaled[2:]):
            assert np.array_equal(np.float32(1024.0) * a, b)
    assert res[0][2].any() and res[0][4].any()


def test_two_calls_give_identical_bits():
    from rcgan_amd import _lib as L
    ctx, g = env()
    pairs, cols, lam = 257, 100, 10.0
    rs, x, xa, w = _case(pairs, cols)
    dev = [_up(ctx, a) for a in (x, xa, w)]
    dx0 = rs.randn(pairs, cols).astype(np.float32)
    res = []
    for _ in range(2):
        loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
        dx, dxa, dw = _up(ctx, dx0), ctx.empty((pairs, cols), L.F32), _up(ctx, np.zeros((pairs, cols)))
        assert call(ctx, g, *dev, lam, loss, term, dx, 1, dxa, dw, pairs, cols) == 0
        res.append([ctx.download(t).view(np.uint32) for t in (loss, term, dx, dxa, dw)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_invalid_arguments_launch_nothing():
    from rcgan_amd import _lib as L
    ctx, g = env()
    pairs, cols = 8, 10
    rs, x, xa, w = _case(pairs, cols)
    xd, xad, wd = [_up(ctx, a) for a in (x, xa, w)]
    loss, term = ctx.empty((1,), L.F32), ctx.empty((1,), L.F32)
    dx, dxa, dw = ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32), ctx.empty((pairs, cols), L.F32)
    fn = ctx.lib.rcgan_pair_consistency_fwd_bwd
    good = dict(pairs=pairs, cols=cols, x=_ptr(xd), xa=_ptr(xad), w=_ptr(wd), lam=10.0, loss=_ptr(loss), term=_ptr(term), dx=_ptr(dx),
                acc=1, dxa=_ptr(dxa), dw=_ptr(dw))
    order = ("pairs", "cols", "x", "xa", "w", "lam", "loss", "term", "dx", "acc", "dxa", "dw")
    cases = [dict(pairs=0), dict(pairs=-1), dict(cols=0), dict(pairs=1 << 16, cols=1 << 15), dict(pairs=(1 << 10) + 1, cols=1 << 10),          # (2^31, and one row past 2^20 elements)
             dict(x=None), dict(xa=None),
             dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf")),
             dict(w=None),                                                  # (a weight gradient without weights)
             dict(x=_ptr(xd, 2)), dict(xa=_ptr(xad, 1)), dict(w=_ptr(wd, 2)), dict(loss=_ptr(loss, 2)), dict(term=_ptr(term, 1)),
             dict(dx=_ptr(dx, 2)), dict(dxa=_ptr(dxa, 3)), dict(dw=_ptr(dw, 2))]
    for c in cases:
        a = dict(good, **c)
        assert fn(ctx.h, *[a[k] for k in order]) == L.EINVALID_ARG, c
    ctx.sync()
    g.check()
    for t in (loss, term, dx, dxa, dw):
        assert g.unwritten(t) == t.size, "a refused call wrote an output"
    # ... and the same arguments, valid, do launch (dx and dwts are ADDED to: given zeros first)
    ctx.check(ctx.lib.rcgan_fill_f32(ctx.h, pairs * cols, _ptr(dx), 0.0))
    ctx.check(ctx.lib.rcgan_fill_f32(ctx.h, pairs * cols, _ptr(dw), 0.0))
    ctx.check(ctx.lib.rcgan_fill_f32(ctx.h, 1, _ptr(loss), 0.0))
    ctx.check(ctx.lib.rcgan_fill_f32(ctx.h, 1, _ptr(term), 0.0))
    assert fn(ctx.h, *[good[k] for k in order]) == 0
    ctx.sync()
    g.check()
    assert g.unwritten(dxa) == 0 and abs(float(ctx.download(loss)[0]) - BR.pair_consistency(x, xa, w, 10.0)["value"]) <= 1e-4


def test_the_op_adds_behind_a_loss_term_and_feeds_the_weights_gradient():
    """ops.pair_consistency behind ops.loss_term: x.grad holds the sum of the two terms' gradients, x_aug.grad and the weight rows'
    gradient (a wts that requires one, as rcgan-u's confusion rows in a generator step) are the references'."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    from tests import head_loss_ref as R
    ctx, g = env()
    pairs, cols, lam = 5, 10, 4.0
    rs, x, xa, w = _case(pairs, cols)
    xd, xad, wd = [_up(ctx, a) for a in (x, xa, w)]
    xd.req = xad.req = wd.req = True
    loss, term = _up(ctx, np.zeros(1)), _up(ctx, np.zeros(1))
    O.loss_term(ctx, L.LOSS_HINGE_FAKE, xd, 1.0, loss, wts=wd)
    O.pair_consistency(ctx, xd, xad, lam, loss, wts=wd, term_acc=term)
    ctx.sync()
    g.check()
    hinge = R.loss_fwd_bwd(R.HINGE_FAKE, x, w, 1.0)
    ref = BR.pair_consistency(x, xa, w, lam)
    np.testing.assert_allclose(ctx.download(loss)[0], hinge[0] + ref["value"], rtol=1e-5)
    np.testing.assert_allclose(ctx.download(term)[0], ref["term"], rtol=1e-5)
    np.testing.assert_allclose(ctx.download(xd.grad), hinge[2] + ref["dx"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ctx.download(xad.grad), ref["dx_aug"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ctx.download(wd.grad), hinge[3] + ref["dwts"], rtol=1e-5, atol=1e-6)
