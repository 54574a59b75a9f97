"""rcgan_lecam_update (csrc/loss.hip) against the float64 restatement of its definition (tests/lecam_ref.py), between guard bands.

Bounds, from the reference's own terms: a batch mean is an fp32 sum of rows * cols terms (cols = ld for a weight-row part, 1 otherwise)
in some fixed order and one division, so it lies within (rows * cols + 4) 2^-24 sum|terms| / rows of the float64 mean.  An anchor after
an update is decay * a + (1 - decay) * m -- two products and a sum, 1 - decay exact in fp32 for the decays used -- so its error is at most
decay * (the anchor's error before) + (1 - decay) * (the mean's bound) + 4 ulp of |decay a| + |(1 - decay) m|; the first update copies the
mean.  The counters are small integers: exact.  The reference runs on the decay as the kernel receives it, float32(decay)."""
import ctypes as C

import numpy as np
import pytest

from tests import lecam_ref as LR
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
_env = {}
OTHER = {1: 2, 2: 1, 63: 65, 64: 64, 65: 63, 1024: 3}           # rows of part b beside `rows` of part a


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


def _ptr(t):
    return C.c_void_p(t.ptr) if t is not None else None


def call(ctx, g, st, logits, rows_a, decay, part_a, part_b, sync=True):
    from rcgan_amd import _lib as L
    lg = ctx.upload(np.ascontiguousarray(logits, np.float32), dtype=L.F32)
    up = lambda p: (ctx.upload(np.asarray(p[0], np.int32)) if p[0] is not None else None,
                    ctx.upload(np.asarray(p[1], np.float32), dtype=L.F32) if p[1] is not None else None)
    (la, wa), (lb, wb) = up(part_a), up(part_b)
    n, ld = logits.shape
    rc = ctx.lib.rcgan_lecam_update(ctx.h, rows_a, n - rows_a, _ptr(lg), ld, _ptr(la), _ptr(wa), _ptr(lb), _ptr(wb), _ptr(st), decay)
    if sync:
        ctx.sync()
        g.check()
    return rc


def _weights(rs, rows, ld):
    """Rows that sum to 1 with negative entries among them (what C^-1 rows look like)."""
    w = rs.randn(rows, ld)
    w += (1.0 - w.sum(1, keepdims=True)) / ld
    return w.astype(np.float32)


def _parts(rs, rows_a, rows_b, ld, swap):
    """ld = 1: neither labels nor weights.  Otherwise one labelled part (labels outside [0, ld) where there are rows to spare) and one
    weight-row part; swap exchanges the two."""
    if ld == 1:
        return (None, None), (None, None), None
    rows_l = rows_b if swap else rows_a
    lab = rs.randint(0, ld, size=rows_l).astype(np.int32)
    bad = None
    if rows_l >= 63:
        bad = np.array([1, 5, 17, rows_l - 1])
        lab[bad] = [-1, ld, 2 ** 31 - 1, -2 ** 31]
    w = _weights(rs, rows_a if swap else rows_b, ld)
    return ((None, w), (lab, None), bad) if swap else ((lab, None), (None, w), bad)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1024])
@pytest.mark.parametrize("ld", [1, 10, 100])
def test_five_updates_against_the_float64_reference(rows, ld):
    from rcgan_amd import _lib as L
    ctx, g = env()
    rows_a, rows_b = rows, OTHER[rows]
    for decay, swap in ((0.0, False), (0.99, False), (0.99, True)):
        if swap and ld == 1:
            continue
        d32 = float(np.float32(decay))
        rs = np.random.RandomState(1000 * rows + 10 * ld + swap)
        ref = LR.new_state()
        st = ctx.upload(np.zeros(8, np.float32), dtype=L.F32)
        err = np.zeros(2)                                          # the anchors' error bounds so far
        for k in range(5):
            part_a, part_b, bad = _parts(rs, rows_a, rows_b, ld, swap)
            lg = (rs.randn(rows_a + rows_b, ld) * 2 + np.where(np.arange(rows_a + rows_b) < rows_a, 1.5, -1.0)[:, None]).astype(np.float32)
            if bad is not None:                                    # rows with a label outside [0, ld): nothing of them is read
                lg[(rows_a if swap else 0) + bad] = np.where(np.arange(ld) % 2, np.inf, -np.inf).astype(np.float32)
            prev = ref
            ref, (ba, bb) = LR.update_from_logits(ref, lg, rows_a, d32, part_a, part_b)
            assert call(ctx, g, st, lg, rows_a, decay, part_a, part_b) == 0
            got = ctx.download(st).astype(np.float64)
            what = "rows %d+%d ld %d decay %g swap %d update %d: got %r want %r" % (rows_a, rows_b, ld, decay, swap, k, got, ref)
            assert np.isfinite(ref).all()
            assert got[LR.UPDATES] == k + 1 and got[LR.SKIPPED] == 0 and got[6] == 0 and got[7] == 0, what
            assert abs(got[LR.MEAN_REAL] - ref[LR.MEAN_REAL]) <= ba and abs(got[LR.MEAN_FAKE] - ref[LR.MEAN_FAKE]) <= bb, what
            means, mb = np.array([ref[LR.MEAN_REAL], ref[LR.MEAN_FAKE]]), np.array([ba, bb])
            if k == 0:
                err = mb
            else:
                err = d32 * err + (1 - d32) * mb + 4 * ULP * (np.abs(d32 * prev[:2]) + np.abs((1 - d32) * means))
            assert (np.abs(got[:2] - ref[:2]) <= err).all(), what + " bound %r" % (err,)
            if decay == 0.0:                                       # decay 0 tracks the batch: the anchors ARE the last means
                assert got[0] == got[LR.MEAN_REAL] and got[1] == got[LR.MEAN_FAKE], what


@pytest.mark.parametrize("poison", [np.inf, -np.inf, np.nan])
def test_a_non_finite_batch_is_skipped_and_the_anchors_keep_their_bits(poison):
    from rcgan_amd import _lib as L
    ctx, g = env()
    rs = np.random.RandomState(3)
    ld, rows_a, rows_b = 10, 65, 64
    start = np.array([0.75, -1.25, 3, 0.5, -0.5, 0, 0, 0], np.float32)
    for where in ("a", "b"):
        st = ctx.upload(start, dtype=L.F32)
        lab = rs.randint(0, ld, size=rows_a).astype(np.int32)
        w = _weights(rs, rows_b, ld)
        lg = rs.randn(rows_a + rows_b, ld).astype(np.float32)
        if where == "a":
            lg[64, lab[64]] = poison                               # (row 64: the second pass of the first wavefront's lane 0)
        else:
            lg[rows_a + 7, 3] = poison
        for k in range(2):
            assert call(ctx, g, st, lg, rows_a, 0.99, (lab, None), (None, w)) == 0
            got = ctx.download(st)
            want = start.copy()
            want[LR.SKIPPED] = k + 1
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (where, k, got)
        ref, _ = LR.update_from_logits(start.astype(np.float64), lg, rows_a, 0.99, (lab, None), (None, w))
        assert ref[LR.SKIPPED] == 1 and ref[LR.UPDATES] == 3
    # a poisoned column that the label does not select is never read: the update goes through
    st = ctx.upload(start, dtype=L.F32)
    lab = np.zeros(rows_a, np.int32)
    lg = rs.randn(rows_a + rows_b, ld).astype(np.float32)
    lg[:rows_a, 1:] = poison
    assert call(ctx, g, st, lg, rows_a, 0.99, (lab, None), (None, w)) == 0
    got = ctx.download(st)
    assert got[LR.UPDATES] == 4 and got[LR.SKIPPED] == 0 and np.isfinite(got).all()


def test_invalid_arguments_launch_nothing():
    from rcgan_amd import _lib as L
    ctx, g = env()
    rs = np.random.RandomState(4)
    ld, ra, rb = 10, 4, 4
    lg = rs.randn(ra + rb, ld).astype(np.float32)
    lab, w = rs.randint(0, ld, size=4).astype(np.int32), _weights(rs, 4, ld)
    good = dict(rows_a=ra, rows_b=rb, ld=ld, a=(lab, None), b=(None, w), decay=0.5)
    cases = [dict(rows_a=0), dict(rows_b=0), dict(rows_a=-1), dict(ld=0), dict(a=(lab, w)), dict(b=(lab, w)), dict(a=(None, None)),
             dict(b=(None, None)), dict(decay=-0.01), dict(decay=1.01), dict(decay=float("nan"))]
    st = ctx.empty((8,), L.F32)
    lgd = ctx.upload(lg, dtype=L.F32)
    labd, wd = ctx.upload(lab), ctx.upload(w, dtype=L.F32)
    dev = lambda p: (_ptr(labd) if p[0] is not None else None, _ptr(wd) if p[1] is not None else None)
    for c in cases:
        a = dict(good, **c)
        rc = ctx.lib.rcgan_lecam_update(ctx.h, a["rows_a"], a["rows_b"], _ptr(lgd), a["ld"], *dev(a["a"]), *dev(a["b"]), _ptr(st), a["decay"])
        assert rc == L.EINVALID_ARG, c
    off = lambda t, k: C.c_void_p(t.ptr + k)
    for args in ((None, ld, _ptr(labd), None, None, _ptr(wd), _ptr(st)), (_ptr(lgd), ld, _ptr(labd), None, None, _ptr(wd), None),
                 (off(lgd, 2), ld, _ptr(labd), None, None, _ptr(wd), _ptr(st)), (_ptr(lgd), ld, off(labd, 1), None, None, _ptr(wd), _ptr(st)),
                 (_ptr(lgd), ld, _ptr(labd), None, None, off(wd, 2), _ptr(st)), (_ptr(lgd), ld, _ptr(labd), None, None, _ptr(wd), off(st, 2))):
        rc = ctx.lib.rcgan_lecam_update(ctx.h, ra, rb, *args, 0.5)
        assert rc == L.EINVALID_ARG, args
    ctx.sync()
    g.check()
    assert g.unwritten(st) == 8, "a refused call wrote the state"
    # ... and the same arguments, valid, do launch
    st2 = ctx.upload(np.zeros(8, np.float32), dtype=L.F32)
    assert ctx.lib.rcgan_lecam_update(ctx.h, ra, rb, _ptr(lgd), ld, _ptr(labd), None, None, _ptr(wd), _ptr(st2), 0.5) == 0
    ctx.sync()
    g.check()
    assert ctx.download(st2)[LR.UPDATES] == 1 and g.unwritten(st) == 8
