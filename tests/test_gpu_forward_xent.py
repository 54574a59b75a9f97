"""The forward-corrected cross-entropy kernel (csrc/classifier.hip, rcgan_softmax_xent_forward_fwd_bwd) against the float64 restatement
of tests/forward_xent_ref.py: loss, gradient, posterior, recovered labels and the count of correct rows over one-coin, dense, sparse and
identity confusion matrices; rows without a usable label; the identity matrix against rcgan_softmax_xent_fwd_bwd bit for bit; refused
arguments; one case inside guard bands with a workspace of exactly the advertised size."""
import ctypes as C

import numpy as np
import pytest

from tests import forward_xent_ref as FR
from tests.gpu_util import FakeParam, assert_close, make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu
WEIGHT = 0.75


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32")
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


_REFS = {}


def _case(rows, cols, kind):
    """(logits, labels, C, float64 reference), computed once per case and left unchanged."""
    key = (rows, cols, kind)
    if key not in _REFS:
        x, lab, Cm = FR.kernel_case(rows, cols, kind)
        for a in (x, lab, Cm):
            a.setflags(write=False)
        _REFS[key] = (x, lab, Cm, FR.forward_xent(x, lab, Cm, WEIGHT))
    return _REFS[key]


def _outputs(ctx, rows, cols):
    from rcgan_amd import _lib as L
    return dict(loss=ctx.persistent((1,), L.F32, fill=0.0), ncor=ctx.persistent((1,), L.F32, fill=0.0),
                post=ctx.persistent((rows, cols), L.F32, fill=-7.0), rec=ctx.persistent((rows,), "i32", fill=-9))


def _check_recovered(got, ref, what):
    """Exact, except that a row whose two largest float64 posteriors differ by less than 1e-4 of the larger may pick either of the two;
    no case may excuse more than 2 % of its rows that way."""
    near, top2 = FR.near_ties(ref["posterior"])
    near &= ref["valid"]
    assert near.mean() <= FR.NEAR_TIE_CAP, (what, near.mean())
    exact = ~near
    assert (got[exact] == ref["recovered"][exact]).all(), (what, np.flatnonzero(got[exact] != ref["recovered"][exact])[:8])
    assert ((got[near] == top2[near, 0]) | (got[near] == top2[near, 1])).all(), what
    return int(near.sum())


@pytest.mark.parametrize("kind", FR.VARIANTS)
@pytest.mark.parametrize("rows,cols", FR.SHAPES)
def test_forward_xent_against_float64(ctx, rows, cols, kind):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    x, lab, Cm, ref = _case(rows, cols, kind)
    bad = ~ref["valid"]
    ctx.new_step()
    ctx.recording = True
    lg = FakeParam(ctx, x.copy())
    labels, ct = ctx.upload(lab), ctx.upload(np.ascontiguousarray(Cm.T), L.F32)
    o = _outputs(ctx, rows, cols)
    O.softmax_xent_forward(ctx, lg.t, labels, ct, WEIGHT, o["loss"], o["ncor"], o["post"], o["rec"])
    got_L, got_n, got_d = float(ctx.download(o["loss"])[0]), float(ctx.download(o["ncor"])[0]), lg.grad(ctx)
    got_p, got_r = ctx.download(o["post"]), ctx.download(o["rec"])
    excused = _check_recovered(got_r, ref, (rows, cols, kind))
    print("forward xent %dx%d %s: loss %.7g (float64 %.7g, diff %.2e), n_correct %d (%d), dlogits max err %.2e of %.2e, posterior max err "
          "%.2e, %d rows without label or support, %d near-tie rows"
          % (rows, cols, kind, got_L, ref["loss"], abs(got_L - ref["loss"]), got_n, ref["n_correct"], np.abs(got_d - ref["dlogits"]).max(),
             np.abs(ref["dlogits"]).max(), np.abs(got_p - ref["posterior"]).max(), int(bad.sum()), excused))
    assert abs(got_L - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"])), (got_L, ref["loss"])
    assert got_n == ref["n_correct"]
    if bad.all():
        assert (got_d == 0).all() and (got_p == 0).all()
    else:
        assert_close(got_d, ref["dlogits"], 2e-5, "dlogits")
        assert_close(got_p, ref["posterior"], 2e-5, "posterior")
        assert np.abs(got_p[~bad].sum(axis=1) - 1.0).max() <= 1e-5
    # a label outside [0, cols) or one that no class emits: zero gradient row, zero posterior row, recovered -1
    assert (got_d[bad] == 0).all() and (got_p[bad] == 0).all() and (got_r[bad] == -1).all() and (got_r[~bad] >= 0).all()
    # the accumulators ADD; evaluation (recording off) writes no gradient; the same bits run to run
    ctx.recording = False
    before = lg.grad(ctx).copy()
    o2 = _outputs(ctx, rows, cols)
    O.softmax_xent_forward(ctx, lg.t, labels, ct, WEIGHT, o["loss"], None, o2["post"], o2["rec"])
    ctx.recording = True
    assert _bits(ctx.download(o["loss"]))[0] == _bits(np.float32(np.float32(got_L) + np.float32(got_L)))[0]
    assert float(ctx.download(o["ncor"])[0]) == ref["n_correct"] and (_bits(lg.grad(ctx)) == _bits(before)).all()
    assert (_bits(ctx.download(o2["post"])) == _bits(got_p)).all() and (ctx.download(o2["rec"]) == got_r).all()
    # the gradient (not the loss) follows rcgan_set_grad_scale, as the other loss kernels' do
    o3 = _outputs(ctx, rows, cols)
    ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 8.0, None))
    try:
        O.softmax_xent_forward(ctx, lg.t, labels, ct, WEIGHT, o3["loss"], o3["ncor"])
    finally:
        ctx.check(ctx.lib.rcgan_set_grad_scale(ctx.h, 1.0, None))
    assert _bits(ctx.download(o3["loss"]))[0] == _bits(np.float32(got_L))[0] and float(ctx.download(o3["ncor"])[0]) == ref["n_correct"]
    if not bad.all():
        assert_close(lg.grad(ctx), 8.0 * ref["dlogits"], 2e-5, "scaled dlogits")
    assert (lg.grad(ctx)[bad] == 0).all()
    # a second full run: every output the same bits
    o4 = _outputs(ctx, rows, cols)
    O.softmax_xent_forward(ctx, lg.t, labels, ct, WEIGHT, o4["loss"], o4["ncor"], o4["post"], o4["rec"])
    assert _bits(ctx.download(o4["loss"]))[0] == _bits(np.float32(got_L))[0]
    assert (_bits(lg.grad(ctx)) == _bits(got_d)).all() and (_bits(ctx.download(o4["post"])) == _bits(got_p)).all()
    assert (ctx.download(o4["rec"]) == got_r).all()


@pytest.mark.parametrize("rows,cols", FR.SHAPES)
def test_identity_matrix_is_the_plain_kernel_bit_for_bit(ctx, rows, cols):
    """C = I and labels in range: m2 = z[label], a = 1, logf(a) = 0, posterior = one-hot, so loss, n_correct and dlogits are those of
    rcgan_softmax_xent_fwd_bwd, the same bits."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    x, lab, Cm = FR.kernel_case(rows, cols, "identity", bad_rows=False)
    assert lab.min() >= 0 and lab.max() < cols
    ctx.new_step()
    ctx.recording = True
    a, b = FakeParam(ctx, x), FakeParam(ctx, x)
    labels, ct = ctx.upload(lab), ctx.upload(np.ascontiguousarray(Cm.T), L.F32)
    la, na = ctx.persistent((1,), L.F32, fill=0.0), ctx.persistent((1,), L.F32, fill=0.0)
    o = _outputs(ctx, rows, cols)
    O.softmax_xent(ctx, a.t, labels, WEIGHT, la, na)
    O.softmax_xent_forward(ctx, b.t, labels, ct, WEIGHT, o["loss"], o["ncor"], o["post"], o["rec"])
    assert _bits(ctx.download(o["loss"]))[0] == _bits(ctx.download(la))[0]
    assert float(ctx.download(o["ncor"])[0]) == float(ctx.download(na)[0])
    da, db = a.grad(ctx), b.grad(ctx)
    assert (_bits(da) == _bits(db)).all(), int((_bits(da) != _bits(db)).sum())
    assert (ctx.download(o["post"]) == np.eye(cols, dtype=np.float32)[lab]).all() and (ctx.download(o["rec"]) == lab).all()


def test_bad_arguments_are_refused_before_any_launch(ctx):
    from rcgan_amd import _lib as L
    rows = 4
    x = ctx.persistent((rows, 1025), L.F32, fill=0.0)
    lab = ctx.persistent((rows,), "i32", fill=0)
    ct = ctx.persistent((1025, 1025), L.F32, fill=0.1)
    loss, dl = ctx.persistent((1,), L.F32, fill=0.0), ctx.persistent((rows, 1025), L.F32, fill=-7.0)
    p = lambda t: C.c_void_p(t.ptr) if t is not None else None
    ws, need = C.c_void_p(ctx.ws_ptr), ctx.lib.rcgan_softmax_xent_workspace_bytes(rows)

    def call(cols=10, logits=x, labels=lab, c=ct, w=ws, wb=ctx.ws_bytes, n=rows):
        return ctx.lib.rcgan_softmax_xent_forward_fwd_bwd(ctx.h, n, cols, p(logits), p(labels), p(c), 1.0, p(loss), None, p(dl), None, None, w, wb)
    for cols in (1, 0, 1025):
        assert call(cols=cols) == L.EUNSUPPORTED_SHAPE, cols
    assert call(logits=None) == L.EINVALID_ARG and call(labels=None) == L.EINVALID_ARG and call(c=None) == L.EINVALID_ARG
    assert call(n=0) == L.EINVALID_ARG
    assert call(wb=need - 1) == L.EWORKSPACE_TOO_SMALL and call(w=None) == L.EWORKSPACE_TOO_SMALL
    ctx.sync()
    assert float(ctx.download(loss)[0]) == 0.0 and (ctx.download(dl) == -7.0).all()          # nothing ran
    assert call(wb=need) == 0                                                                 # ... and the exact size is enough
    ctx.sync()
    assert float(ctx.download(loss)[0]) > 0.0 and np.isfinite(ctx.download(dl)[:, :10]).all()


def test_inside_guard_bands_with_the_exact_workspace():
    """Logits, labels, ct, the three outputs and the scalars between 0xFF margins, the workspace exactly
    rcgan_softmax_xent_workspace_bytes(rows) between margins of its own: everything is written, nothing outside is touched.  130 rows
    = 33 workgroups, the last with two idle wavefronts; the sparse matrix brings rows without support."""
    from rcgan_amd import _lib as L
    rows, cols, kind = 130, 100, "sparse"
    x, lab, Cm = FR.kernel_case(rows, cols, kind)
    ref = FR.forward_xent(x, lab, Cm, WEIGHT)
    bad = ~ref["valid"]
    assert bad.any() and not bad.all()
    ctx = make_ctx("f32", arena=1 << 20)          # (its own arena is replaced by the guarded one)
    p = lambda t: C.c_void_p(t.ptr)
    try:
        with guarded(ctx) as g:
            need = ctx.lib.rcgan_softmax_xent_workspace_bytes(rows)
            with g.workspace(need):
                assert ctx.ws_bytes == need
                ctx.new_step()
                xd, labd, ctd = ctx.upload(x, L.F32), ctx.upload(lab), ctx.upload(np.ascontiguousarray(Cm.T), L.F32)
                dl, post, rec = ctx.empty((rows, cols), L.F32), ctx.empty((rows, cols), L.F32), ctx.empty((rows,), "i32")
                loss, ncor = ctx.persistent((1,), L.F32, fill=0.0), ctx.persistent((1,), L.F32, fill=0.0)
                ctx.check(ctx.lib.rcgan_softmax_xent_forward_fwd_bwd(ctx.h, rows, cols, p(xd), p(labd), p(ctd), WEIGHT, p(loss), p(ncor), p(dl),
                                                                     p(post), p(rec), C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
                ctx.sync()
                g.check()
                assert g.unwritten(dl) == 0 and g.unwritten(post) == 0
                assert g.unwritten(rec) == int(bad.sum())          # (-1, the answer for a row without label or support, is the fill pattern)
                got_L, got_n = float(ctx.download(loss)[0]), float(ctx.download(ncor)[0])
                assert abs(got_L - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"])) and got_n == ref["n_correct"]
                assert_close(ctx.download(dl), ref["dlogits"], 2e-5, "dlogits")
                assert_close(ctx.download(post), ref["posterior"], 2e-5, "posterior")
                _check_recovered(ctx.download(rec), ref, "guarded")
                ctx.sync()
                g.check()
    finally:
        ctx.close()
