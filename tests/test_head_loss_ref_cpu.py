"""tests/head_loss_ref.py checked without a GPU: every adjoint against central differences in float64, the loss / softmax / batch-norm
values against oracle/nn.py, and the two fp32 forms of the saturated sigmoid cross-entropy gradient against the per-element bound the
GPU tests use -- the form of csrc/loss.hip meets it over x in [-80, 80], the subtracted form it replaced does not."""
import numpy as np
import pytest

from oracle import nn
from tests import head_loss_ref as R


def _numgrad(f, x, h=1e-6):
    """Central differences of the scalar f at x (float64), one element at a time."""
    x = np.array(x, np.float64)
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        k = it.multi_index
        keep = x[k]
        x[k] = keep + h
        fp = f(x)
        x[k] = keep - h
        fm = f(x)
        x[k] = keep
        g[k] = (fp - fm) / (2 * h)
    return g


def _close(a, b, tol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def _away_from_kinks(rs, shape, kinks=(0.0,), gap=1e-3):
    x = rs.randn(*shape) * 1.5
    for k in kinks:
        x = np.where(np.abs(x - k) < gap, x + 3 * gap, x)
    return x


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU])
def test_act_meanhw_adjoint(act):
    rs = np.random.RandomState(act)
    x, w = _away_from_kinks(rs, (2, 5, 3)), rs.randn(2, 3)
    feat, mag = R.act_meanhw_fwd(x, act)
    assert (mag >= np.abs(feat) - 1e-15).all()
    _close(R.act_meanhw_bwd(x, w, act), _numgrad(lambda v: (R.act_meanhw_fwd(v, act)[0] * w).sum(), x))
    zero = np.zeros((1, 2, 2))
    assert (R.act_meanhw_bwd(zero, np.ones((1, 2)), R.ACT_RELU) == 0).all()                 # x = 0: the negative side
    assert np.allclose(R.act_meanhw_bwd(zero, np.ones((1, 2)), R.ACT_LRELU), 0.2 / 2)


def test_gather_scatter_are_adjoint():
    rs = np.random.RandomState(1)
    table, idx, src = rs.randn(7, 3), np.array([2, 2, 5, 0]), rs.randn(4, 3)
    tg, mag = R.scatter_add_rows(src, idx, 7)
    assert np.isclose((R.gather_rows(table, idx) * src).sum(), (table * tg).sum())
    assert (tg[[1, 3, 4, 6]] == 0).all() and np.allclose(tg[2], src[0] + src[1]) and np.allclose(mag[2], np.abs(src[0]) + np.abs(src[1]))
    prev = rs.randn(7, 3)
    tg2, _ = R.scatter_add_rows(src, idx, 7, prev)
    assert np.array_equal(tg2[[1, 3, 4, 6]], prev[[1, 3, 4, 6]]) and np.allclose(tg2, prev + tg)


def test_proj_logit_adjoints():
    rs = np.random.RandomState(2)
    feat, psi, emb, g = rs.randn(3, 5), rs.randn(3), rs.randn(3, 5), rs.randn(3)
    dfeat, mag, dpsi, demb = R.proj_logit_bwd(feat, emb, g)
    _close(dfeat, _numgrad(lambda v: (R.proj_logit_fwd(v, psi, emb)[0] * g).sum(), feat))
    _close(demb, _numgrad(lambda v: (R.proj_logit_fwd(feat, psi, v)[0] * g).sum(), emb))
    _close(dpsi, _numgrad(lambda v: (R.proj_logit_fwd(feat, v, emb)[0] * g).sum(), psi))
    assert np.allclose(R.proj_logit_fwd(feat, None, emb)[0], (feat * emb).sum(1))
    prev = rs.randn(3, 5)
    d2, m2, _, _ = R.proj_logit_bwd(feat, emb, g, prev)
    assert np.allclose(d2, dfeat + prev) and np.allclose(m2, mag + np.abs(prev))


def test_proj_logit_all_adjoints():
    rs = np.random.RandomState(3)
    feat, psi, E, g = rs.randn(3, 5), rs.randn(3), rs.randn(4, 5), rs.randn(3, 4)
    g[1] = 0.0
    (dfeat, mf), (dpsi, mp), (dE, mE) = R.proj_logit_all_bwd(feat, E, g)
    f = lambda a, b, c: (R.proj_logit_all_fwd(a, b, c)[0] * g).sum()
    _close(dfeat, _numgrad(lambda v: f(v, psi, E), feat))
    _close(dpsi, _numgrad(lambda v: f(feat, v, E), psi))
    _close(dE, _numgrad(lambda v: f(feat, psi, v), E))
    assert (dfeat[1] == 0).all() and dpsi[1] == 0
    assert (mf >= np.abs(dfeat) - 1e-15).all() and (mp >= np.abs(dpsi) - 1e-15).all() and (mE >= np.abs(dE) - 1e-15).all()
    lg, mag = R.proj_logit_all_fwd(feat, psi, E)
    assert np.allclose(lg, psi[:, None] + feat @ E.T) and (mag >= np.abs(lg) - 1e-15).all()


@pytest.mark.parametrize("kind", [R.HINGE_REAL, R.HINGE_FAKE, R.NEG_MEAN, R.CE_ONES, R.CE_ZEROS])
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_adjoints(kind, weighted):
    rs = np.random.RandomState(kind * 2 + weighted)
    x = _away_from_kinks(rs, (4, 3), kinks=(-1.0, 1.0))
    wts = rs.rand(4, 3) + 0.1 if weighted else None
    weight = -2.0
    val, mag, dx, dw = R.loss_fwd_bwd(kind, x, wts, weight)
    assert mag >= abs(val) - 1e-15
    _close(dx, _numgrad(lambda v: R.loss_fwd_bwd(kind, v, wts, weight)[0], x))
    if weighted:
        _close(dw, _numgrad(lambda v: R.loss_fwd_bwd(kind, x, v, weight)[0], wts))
    _, _, dx512, dw512 = R.loss_fwd_bwd(kind, x, wts, weight, scale=512.0)
    assert np.array_equal(dx512, 512.0 * dx) and np.array_equal(dw512, 512.0 * dw)
    # 1-D input = one column
    assert R.loss_fwd_bwd(kind, x[:, 0], None, weight)[0] == R.loss_fwd_bwd(kind, x[:, :1], None, weight)[0]


def test_hinge_at_the_kink():
    """x = +-1 exactly: term and derivative are 0 (TF's ReLU gradient at 0)."""
    for kind, x in ((R.HINGE_REAL, 1.0), (R.HINGE_FAKE, -1.0)):
        t, d = R.loss_term(kind, np.array([x]))
        assert t[0] == 0 and d[0] == 0


def test_bce_onehot_adjoint():
    rs = np.random.RandomState(5)
    x, lab = rs.randn(4, 6) * 3, np.array([0, 5, 2, 2])
    val, mag, dx = R.bce_onehot_fwd_bwd(x, lab, 0.5)
    _close(dx, _numgrad(lambda v: R.bce_onehot_fwd_bwd(v, lab, 0.5)[0], x))
    Z = np.eye(6)[lab]
    assert np.isclose(val, 0.5 * nn.sigmoid_ce_logits(x, Z).mean()) and mag >= abs(val)
    _close(dx, 0.5 * nn.sigmoid_ce_logits_bwd(x, Z) / x.size, 1e-12)


def test_sigmoid_terms_match_the_oracle():
    x = np.linspace(-20, 20, 401)
    for z in (0.0, 1.0):
        assert np.allclose(R.sigmoid_ce(x, z), nn.sigmoid_ce_logits(x, z), rtol=1e-13, atol=0)
        # (the oracle's gradient is the subtracted form in float64: 1e-16 absolute, which is 5e-8 of e^-20)
        assert np.allclose(R.sigmoid_ce_grad(x, z), nn.sigmoid_ce_logits_bwd(x, z), rtol=1e-6, atol=0)
    # the stable form against its series far out, where the subtracted one has nothing left: sigmoid(x) - 1 = -e^-x (1 - e^-x + ...)
    assert np.isclose(R.sigmoid_ce_grad(80.0, 1.0), -np.exp(-80.0), rtol=1e-15)
    assert np.isclose(R.sigmoid_ce_grad(-80.0, 0.0), np.exp(-80.0), rtol=1e-15)


def test_softmax_matches_the_oracle_and_its_adjoint():
    rs = np.random.RandomState(6)
    l = rs.randn(5, 7) * 3
    l[1] = 2.5
    l[2] += 1e4
    p, bound = R.softmax_rows_fwd(l)
    assert np.allclose(p, nn.softmax_rows(l), rtol=1e-14) and np.allclose(p.sum(1), 1.0) and (bound > 0).all()
    dp = rs.randn(5, 7).astype(np.float32).astype(np.float64)
    _close(p * (dp - (dp * p).sum(1, keepdims=True)), _numgrad(lambda v: (R.softmax_rows_fwd(v)[0] * dp).sum(), l), 1e-5)
    p = p.astype(np.float32).astype(np.float64)             # (the adjoint takes the fp32 values the forward pass stored)
    _close(R.softmax_rows_bwd(p, dp), nn.softmax_rows_bwd(dp, p), 1e-14)
    prev = rs.randn(5, 7)
    assert np.allclose(R.softmax_rows_bwd(p, dp, prev), R.softmax_rows_bwd(p, dp) + prev)
    # a saturated row: p = 1 at the dominant entry in fp32, whose gradient is minus the others' share -- float64 alone returns 0 or noise
    ps = np.array([[1.0, 2.0 ** -70, 2.0 ** -72]])
    ds = np.array([[0.75, -0.5, 3.0]])
    want = -(ds[0, 1] * ps[0, 1] + ds[0, 2] * ps[0, 2])
    assert R.softmax_rows_bwd(ps, ds)[0, 0] == want and want != 0
    assert nn.softmax_rows_bwd(ds, ps)[0, 0] != want


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH, R.ACT_SIGMOID])
def test_bn_infer_and_adjoint(act):
    rs = np.random.RandomState(7 + act)
    x = rs.randn(6, 4)
    g, b, mm, mv = rs.rand(4) + 0.5, rs.randn(4), rs.randn(4), rs.rand(4)
    mv[0] = 0.0                                         # eps alone in the root
    eps = 1e-5
    y, pre = R.bn_infer(x, g, b, mm, mv, eps, act)
    assert np.allclose(pre, nn.batch_norm_infer(x, g, b, mm, mv, eps), rtol=1e-13)
    x = np.where(np.abs(pre) < 1e-3, x + 0.1, x)       # (away from the kink of ReLU / leaky ReLU)
    y, pre = R.bn_infer(x, g, b, mm, mv, eps, act)
    dy = rs.randn(6, 4)
    _close(R.bn_infer_bwd(y, dy, g, mv, eps, act), _numgrad(lambda v: (R.bn_infer(v, g, b, mm, mv, eps, act)[0] * dy).sum(), x), 1e-5)
    prev = rs.randn(6, 4)
    assert np.allclose(R.bn_infer_bwd(y, dy, g, mv, eps, act, prev), R.bn_infer_bwd(y, dy, g, mv, eps, act) + prev)


# ---------------------------------------------------------------------------------------------------- the bound and the two fp32 forms
X_SAT = np.concatenate([np.linspace(-80, 80, 6401), [10.0, 12.0, 17.0, 30.0, 80.0, -10.0, -12.0, -17.0, -30.0, -80.0]])


def test_fp32_stable_gradient_form_meets_the_bound():
    """-1 / (1 + expf(x)) in fp32 against float64, per element: within 1e-5 |ref| + 1e-37 everywhere in [-80, 80] (it is within a few
    1e-7: one exponential, one addition, one division)."""
    ref = R.sigmoid_ce_grad(X_SAT.astype(np.float32), 1.0)
    for form in (R.ce_ones_grad_f32_stable, R.ce_ones_grad_f32_kernel):          # written out literally / as the kernel evaluates it
        got = form(X_SAT)
        assert got.dtype == np.float32
        assert R.worst(got, ref, R.elem_bound(ref)) <= 1.0
        assert (np.abs(got - ref) <= 1e-6 * np.abs(ref) + 1e-37).all()
    # CE_ZEROS is the mirror image: 1 / (1 + expf(-x))
    ref0 = R.sigmoid_ce_grad(X_SAT.astype(np.float32), 0.0)
    assert R.worst(-R.ce_ones_grad_f32_stable(-X_SAT), ref0, R.elem_bound(ref0)) <= 1.0


def test_fp32_subtracted_gradient_form_fails_the_bound():
    """sigmoid(x) - 1 in fp32: 5e-4 off at x = 10, about 1 % at 12, exactly 0 (100 %) from 17 up -- the bound rejects it."""
    ref = R.sigmoid_ce_grad(X_SAT.astype(np.float32), 1.0)
    got = R.ce_ones_grad_f32_subtracted(X_SAT)
    assert R.worst(got, ref, R.elem_bound(ref)) > 1.0
    rel = lambda x: abs(float(R.ce_ones_grad_f32_subtracted([x])[0]) / float(R.sigmoid_ce_grad(np.float32(x), 1.0)) - 1.0)
    assert rel(10.0) > 1e-5 and rel(12.0) > 1e-3
    for x in (17.0, 30.0, 80.0):
        assert R.ce_ones_grad_f32_subtracted([x])[0] == 0.0


def test_bounds_helpers():
    assert R.worst(np.array([1.0, np.nan]), np.array([1.0, 1.0]), 1.0) == np.inf
    assert R.worst(np.array([0.0]), np.array([0.0]), np.array([0.0])) == 0.0
    assert R.worst(np.array([1e-40]), np.array([0.0]), R.elem_bound(np.array([0.0]))) < 1.0
    assert np.isclose(R.sum_bound(128, 2.0), 132 * 2.0 ** -24 * 2.0)
