"""Batch norm (csrc/bn.hip, routes decided in csrc/bn_plan.h) at its label, shape and numeric edges, through the C ABI, inside guard bands
(tests/guard.py) and with the workspace sized by the query function, against float64 numpy.

Reference: bn_ref / bn_ref_bwd below -- the formulas of test_gpu_many_classes_ops._bn_ref (tests/test_bn_plan_cpu.py checks that the two
agree) with the per-class sums taken per sample first, so that a 17 Mi element tensor does not go through np.add.at row by row.  Activation
masks come from the kernel's own y, as in the existing tests.

Tolerances are the project's: TOL[mode] for y and dx, max(TOL, 2e-5) for freshly written dgamma / dbeta, 1e-4 for accumulated ones (as in
test_cond_bn_many_classes) -- but applied PER LABEL ROW (dgamma, dbeta) and PER CHANNEL (y, dx), each against its own max|ref|, so that a
class with one sample is not hidden behind a class with a thousand.  A row whose reference is identically zero must be exactly zero.

Why each case reaches its route: PLAN_CLAIMS lists, for every case table below, the planner call it amounts to and the route / branch it
is meant to reach; tests/test_bn_plan_cpu.py runs tests/tools/bn_plan_sweep.cpp on those lines and asserts them, without a GPU.

  table          shapes (n, rows per sample, c)                         reaches
  -------------  -----------------------------------------------------  ---------------------------------------------------------------
  PACK_CASES     c 64 / 128, 1 .. 16 rows per sample, n = 32, 96, 160   labelled BN_COLUMN backward, nsub = 32 / rows samples per workgroup
                                                                        ("packed"): one, two and three 64-sample finisher rounds, the last ragged
                 n = 33, 161; 9 rows per sample                         n % nsub != 0 or 32 % rows != 0: one short sample per workgroup ("short")
  LABEL_SHAPES   (48,16,64) (6,64,128)                                  BN_COLUMN packed / a sample split into two groups ("split")
                 (48,9,24) (48,9,200)                                   BN_VEC (c % 8 == 0, no power of two >= 64)
                 (48,9,20) (48,9,3)                                     BN_SCALAR
                 the same with K = 17                                   BN_WIDE (vector partials for c % 8 == 0, scalar otherwise)
  TREE_SHAPE     (32,1024,128): 4 Mi elements                           BN_TREE with RCGAN_BN_TREE_MIN of tests/conftest.py, 16 groups per sample
  STRIDE_CASES   (410,256,20) (46,1024,360) (66,1024,256)               scalar / vector / fused apply kernels, forward and backward: 8192
                                                                        workgroups and a second grid stride (just past 8192 x 256 items)
  STATS_ROWS     rows 1, 2, 511 .. 513 and the fp32 group-size steps    rcgan_bn_stats on BN_COLUMN (c 64, 2048), BN_VEC (24), BN_SCALAR (20);
                 of bn_group_rows (HALVINGS, from the sweep's output)   BN_TREE at (4096,1024)
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests.guard import guarded
from tests.gpu_util import half_round, make_ctx

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 1e-2, "f16": 3e-3}          # test_gpu_ops.TOL
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EWORKSPACE_TOO_SMALL = -3


# ---------------------------------------------------------------------------------------------------- case tables (no GPU needed to read them)
PACK_CASES = [(c, rps) for c in (64, 128) for rps in (1, 2, 4, 8, 16)] + [(64, 9)]


def pack_ns(rps):
    return [32, 96, 160, 33, 161] if 32 % rps == 0 else [32, 33]


LABEL_SHAPES = {"column_packed": (48, 16, 64), "column_split": (6, 64, 128), "vec24": (48, 9, 24), "vec200": (48, 9, 200),
                "scalar20": (48, 9, 20), "scalar3": (48, 9, 3)}
LABEL_ROUTES = {"column_packed": ("COLUMN", "packed"), "column_split": ("COLUMN", "split"), "vec24": ("VEC", "sample"), "vec200": ("VEC", "sample"),
                "scalar20": ("SCALAR", "sample"), "scalar3": ("SCALAR", "sample")}
LABEL_KS = (1, 2, 16, 17)
TREE_SHAPE = (32, 1024, 128)
STRIDE_CASES = {"scalar": (410, 256, 20), "vec": (46, 1024, 360), "fused": (66, 1024, 256)}
STRIDE_APPLY = {"scalar": "SCALAR", "vec": "VEC", "fused": "COLUMN"}
# rows at which bn_group_rows changes the fp32 rows per group (the "halving" lines of bn_plan_sweep sweep): c -> (rows, below, at)
HALVINGS = {20: (16384, 32, 64), 24: (16384, 32, 64), 64: (16384, 32, 64), 2048: (512, 32, 64)}
STATS_ROUTES = {64: "COLUMN", 2048: "COLUMN", 24: "VEC", 20: "SCALAR"}
STATS_TREE = (4096, 1024)
STATS_ROWS = {c: sorted({1, 2, 511, 512, 513, HALVINGS[c][0] - 1, HALVINGS[c][0], HALVINGS[c][0] + 1}) for c in STATS_ROUTES}
SEGMENT_LINES_CASE = (8, (1, 4, 2048))          # nseg x c / 64 = 256 counter lines exactly: still one launch
# a labelled backward one sample past what the query function covers (the header of rcgan_bn_bwd; the sweep's first_exceed lines)
FIRST_EXCEED = {("COLUMN", 1, 64, 10): 8210, ("VEC", 1, 24, 10): 8205, ("SCALAR", 1, 20, 10): 8211, ("WIDE", 1, 128, 17): 8210}
CONTRACT_CASE = ("COLUMN", 1, 64, 10)
QUERY_SHAPES = [(1, 1, 1), (48 * 9, 24, 16), (160 * 16, 128, 10), (1 << 20, 256, 17), (66 * 1024, 256, 10), (3 << 20, 64, 1024), (8210, 64, 10)]


def query_bytes(rows, c, n_labels=1):
    """rcgan_bn_workspace_bytes_labels restated (as in tests/tools/bn_plan_sweep.cpp); test_query_formulas pins it to the library."""
    ng = 2 * max((rows + 511) // 512 + 1, 4096)
    return (ng * 2 * c + 4 * c + 2 * 16 * c) * 4 + 256 + (2 * (n_labels - 16) * c * 4 if n_labels > 16 else 0)


def plan_claims():
    """(case id, "op nseg n rps c n_labels labelled dtype ws" for bn_plan_sweep cases, {field: expected value})."""
    out = []
    for c, rps in PACK_CASES:
        for n in pack_ns(rps):
            packed = 32 % rps == 0 and n % (32 // rps) == 0
            exp = {"route": "COLUMN", "branch": "packed" if packed else "short", "nsub": str(32 // rps if packed else 1)}
            out.append(("pack c%d rps%d n%d" % (c, rps, n), "BWD 1 %d %d %d 10 1 1 query" % (n, rps, c), exp))
    for name, (n, rps, c) in LABEL_SHAPES.items():
        for K in LABEL_KS:
            route, branch = LABEL_ROUTES[name] if K <= 16 else ("WIDE", "wide_vec" if c % 8 == 0 else "wide_scalar")
            out.append(("labels %s K%d" % (name, K), "BWD 1 %d %d %d %d 1 1 query" % (n, rps, c, K), {"route": route, "branch": branch}))
            out.append(("labels %s K%d fwd" % (name, K), "APPLY 1 %d %d %d %d 1 1 query" % (n, rps, c, K),
                        {"apply": LABEL_ROUTES[name][0]}))
    n, rps, c = TREE_SHAPE
    out.append(("tree", "BWD 1 %d %d %d 16 1 1 query" % (n, rps, c), {"route": "TREE", "branch": "split", "gps": "16", "apply": "COLUMN"}))
    for name, (n, rps, c) in STRIDE_CASES.items():
        for op in ("APPLY", "BWD"):
            out.append(("stride %s %s" % (name, op), "%s 1 %d %d %d 10 1 1 query" % (op, n, rps, c),
                        {"apply": STRIDE_APPLY[name], "apply_grid": "8192", "strides": "2"}))
    for c, rows_list in STATS_ROWS.items():
        for rows in rows_list:
            exp = {"route": STATS_ROUTES[c], "branch": "groups"}
            h = HALVINGS[c]
            if rows in (h[0] - 1, h[0]):
                exp["rpg"] = str(h[1] if rows < h[0] else h[2])
            out.append(("stats c%d rows%d" % (c, rows), "STATS 1 1 %d %d 1 0 0 query" % (rows, c), exp))
    out.append(("stats tree", "STATS 1 1 %d %d 1 0 1 query" % STATS_TREE, {"route": "TREE"}))
    nseg, (n, rps, c) = SEGMENT_LINES_CASE
    out.append(("segments 256 lines", "STATS_SEG %d %d %d %d 10 1 1 query" % (nseg, n, rps, c), {"per_segment": "0", "route": "COLUMN", "apply": "COLUMN"}))
    out.append(("segments 9 x 2048", "STATS_SEG 9 1 4 2048 10 1 1 query", {"per_segment": "1", "apply": "COLUMN"}))
    out.append(("one segment", "APPLY_SEG 1 6 16 64 10 1 1 query", {"per_segment": "1", "apply": "COLUMN"}))
    out.append(("stats segments", "STATS_SEG 3 1 513 64 10 1 1 query", {"per_segment": "0", "route": "COLUMN"}))
    for (route, rps, c, K), n in FIRST_EXCEED.items():
        out.append(("contract %s" % route, "BWD 1 %d %d %d %d 1 1 query" % (n, rps, c, K), {"route": route if route != "VEC" else "SCALAR"}))
    return out


# every branch the tables above are meant to reach, as (route, branch) of a reduction or ("apply", family, strides): tests/test_bn_plan_cpu.py
# asserts that the claims as a whole cover them
BRANCHES = [("COLUMN", "packed"), ("COLUMN", "short"), ("COLUMN", "split"), ("COLUMN", "groups"), ("VEC", "sample"), ("VEC", "groups"),
            ("SCALAR", "sample"), ("SCALAR", "groups"), ("TREE", "split"), ("TREE", "groups"), ("WIDE", "wide_vec"), ("WIDE", "wide_scalar"),
            ("apply", "SCALAR", "2"), ("apply", "VEC", "2"), ("apply", "COLUMN", "2")] + [("nsub", str(k)) for k in (2, 4, 8, 16, 32)]


# ---------------------------------------------------------------------------------------------------- float64 reference
def bn_ref(x, labels, gamma, beta, eps=1e-5):
    """x [n, rps, c] -> batch statistics over all rows, xhat and the pre-activation gamma[l] * xhat + beta[l], all float64."""
    n, rps, c = x.shape
    xr = x.reshape(-1, c).astype(np.float64)
    mu, var = xr.mean(0), xr.var(0)
    rs = 1.0 / np.sqrt(var + eps)
    xh = ((xr - mu) * rs).reshape(n, rps, c)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    pre = xh * g64[lab][:, None, :] + b64[lab][:, None, :]
    return SimpleNamespace(mu=mu, var=var, rs=rs, xh=xh, pre=pre, lab=lab, g64=g64, rows=n * rps)


def act_ref(act, pre):
    return pre if act == ACT_NONE else np.maximum(pre, 0.0) if act == ACT_RELU else np.maximum(pre, 0.2 * pre)


def mask_of(act, y):
    """The activation's derivative as the kernels take it: from the sign of the (kernel's own) output."""
    return np.ones_like(y, np.float64) if act == ACT_NONE else np.where(y > 0, 1.0, 0.0 if act == ACT_RELU else 0.2)


def bn_ref_bwd(r, dy, mask, K):
    """dgamma[l] = sum over class-l rows of dy' * xhat, dbeta[l] = sum dy', dx through the batch statistics (dy' = dy * mask)."""
    g = dy.astype(np.float64) * mask
    c = g.shape[-1]
    dgam, dbet = np.zeros((K, c)), np.zeros((K, c))
    np.add.at(dgam, r.lab, (g * r.xh).sum(1))
    np.add.at(dbet, r.lab, g.sum(1))
    g *= r.g64[r.lab][:, None, :]                                   # dxhat
    m1, m2 = g.reshape(-1, c).mean(0), (g * r.xh).reshape(-1, c).mean(0)
    dx = r.rs * (g - m1 - r.xh * m2)
    return dx, dgam, dbet


def assert_rows_close(a, ref, tol, what, extra=None):
    """a, ref [R, m]: every row R against its own scale, |a - ref| <= tol * max|ref[R]|; rows whose reference is all zero: exactly zero.
    extra [R]: added to the scale (the size of the operands where the result is their small difference: the statistics edges)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    scale = np.abs(ref).max(1) + (0.0 if extra is None else np.asarray(extra, np.float64))
    err = np.abs(a - ref).max(1)
    zero = scale == 0
    assert (a[zero] == 0).all(), "%s: rows %s have a zero reference and are not exactly zero" % (what, np.nonzero(zero & (np.abs(a).max(1) != 0))[0][:8])
    rel = np.where(zero, 0.0, err / np.where(zero, 1.0, scale))
    k = int(rel.argmax())
    assert rel[k] <= tol, "%s: row %d max err %.3e of its max|ref| = %.3e > %.1e (%d of %d rows over)" % (what, k, rel[k], scale[k], tol, (rel > tol).sum(), len(rel))
    return float(rel[k])


def assert_channels_close(a, ref, tol, what, extra=None):
    c = ref.shape[-1]
    return assert_rows_close(np.asarray(a).reshape(-1, c).T, np.asarray(ref).reshape(-1, c).T, tol, what, extra)


# One-pass fp32 statistics: the kernels add x and x * x in fp32 along chains of at most 512 / 4 + 4 = 132 terms (a 512-row group over the 4
# row lanes of the scalar kernel, then the lanes; the vector and column kernels have shorter chains) and combine the groups in fp64.  A
# chain of m terms is off by at most m * 2^-24 * sum|terms|, so mean is off by at most CHAIN_U * E|x| and the variance by at most
# CHAIN_U * (E[x^2] + 2 |mean| E|x|); rstd = (var + eps)^-1/2 turns a variance error dv into a relative error dv / (2 (var + eps)).
# The 132 restates the kernels' grouping as it stands (bn_group_rows: at most 512 rows per group; bn_partial_kernel: 4 row lanes): a
# regrouping of the statistics kernels that lengthens their fp32 chains has to revisit this constant, one that shortens them may lower it.
CHAIN_U = 132 * 2.0 ** -24


def assert_stats_close(mean, rstd, x2, eps, what):
    """mean, rstd against float64 per channel: the project's fp32 tolerance plus the bound above (which is what decides a channel whose
    spread is small beside its mean, a two-row batch among them)."""
    x64 = x2.astype(np.float64)
    mu, var, ax, x2m = x64.mean(0), x64.var(0), np.abs(x64).mean(0), (x64 * x64).mean(0)
    rs = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    em = np.abs(mean - mu) - (TOL["f32"] * np.abs(mu).max() + CHAIN_U * ax)
    er = np.abs(rstd - rs) / rs - (TOL["f32"] + CHAIN_U * (x2m + 2 * np.abs(mu) * ax) / (2 * (var + np.float64(np.float32(eps)))))
    assert np.isfinite(mean).all() and np.isfinite(rstd).all(), what
    assert em.max() <= 0, "mean %s: channel %d off by %.3e" % (what, em.argmax(), np.abs(mean - mu)[em.argmax()])
    assert er.max() <= 0, "rstd %s: channel %d off by %.3e of %.3e" % (what, er.argmax(), np.abs(rstd - rs)[er.argmax()], rs[er.argmax()])


# ---------------------------------------------------------------------------------------------------- contexts
@pytest.fixture(scope="module")
def _contexts():
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx)
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


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _ws(ctx):
    return C.c_void_p(ctx.ws_ptr), ctx.ws_bytes


def _forward(ctx, x, labels, gamma, beta, K, act, eps=1e-5):
    """rcgan_bn_stats + rcgan_bn_apply_fwd; the device tensors stay for the backward calls."""
    from rcgan_amd import _lib as L
    n, rps, c = x.shape
    d = SimpleNamespace(n=n, rps=rps, c=c, K=K, act=act)
    d.x = ctx.upload(x.reshape(n * rps, c), ctx.act_dtype)
    d.y = ctx.empty((n * rps, c), ctx.act_dtype)
    d.lab = ctx.upload(np.asarray(labels).astype(np.int32)) if labels is not None else None
    d.g, d.b = ctx.upload(gamma, L.F32), ctx.upload(beta, L.F32)
    d.mean, d.rstd = ctx.empty((c,), L.F32), ctx.empty((c,), L.F32)
    ws, wsb = _ws(ctx)
    ctx.check(ctx.lib.rcgan_bn_stats(ctx.h, n * rps, c, d.x.dtype, _p(d.x), eps, _p(d.mean), _p(d.rstd), None, None, 0.0, ws, wsb))
    ctx.check(ctx.lib.rcgan_bn_apply_fwd(ctx.h, n, rps, c, K, d.x.dtype, _p(d.x), _p(d.lab), _p(d.g), _p(d.b), _p(d.mean), _p(d.rstd), act, _p(d.y), ws, wsb))
    assert ctx.guard.unwritten(d.y) == 0, "the forward left elements of y unwritten"
    d.yh = ctx.download(d.y).astype(np.float64).reshape(n, rps, c)
    return d


def _backward(ctx, d, dy_dev, via, acc, acc_dx, pre, dx0):
    """rcgan_bn_bwd (mask read from y) or rcgan_bn_bwd2 (beta passed: mask recomputed from x on the fused routes) -> dx, dgamma, dbeta."""
    from rcgan_amd import _lib as L
    rows, c = d.n * d.rps, d.c
    dx = ctx.upload(dx0.reshape(rows, c), ctx.act_dtype) if dx0 is not None else ctx.empty((rows, c), ctx.act_dtype)
    dg, db = ctx.upload(pre[0], L.F32), ctx.upload(pre[1], L.F32)
    ws, wsb = _ws(ctx)
    if via == "y":
        ctx.check(ctx.lib.rcgan_bn_bwd(ctx.h, d.n, d.rps, c, d.K, d.x.dtype, _p(d.x), _p(d.y), _p(dy_dev), _p(d.lab), _p(d.g), _p(d.mean), _p(d.rstd),
                                       d.act, _p(dx), acc_dx, _p(dg), _p(db), acc, ws, wsb))
    else:
        ctx.check(ctx.lib.rcgan_bn_bwd2(ctx.h, d.n, d.rps, c, d.K, d.x.dtype, _p(d.x), _p(d.y), _p(dy_dev), _p(d.lab), _p(d.g), _p(d.b), _p(d.mean),
                                        _p(d.rstd), d.act, _p(dx), acc_dx, _p(dg), _p(db), acc, ws, wsb))
    return ctx.download(dx).astype(np.float64).reshape(d.n, d.rps, c), ctx.download(dg).astype(np.float64), ctx.download(db).astype(np.float64)


def _check_bwd(mode, got, ref, pre, dx0, acc, present, what):
    """got, ref = (dx, dgamma, dbeta); pre = the buffers the call found; per label row and per channel."""
    dx, dg, db = got
    dxr, dgr, dbr = ref
    tol = TOL[mode]
    if acc:
        assert np.array_equal(dg[~present], pre[0][~present].astype(np.float64)), "absent classes keep their bits (dgamma) " + what
        assert np.array_equal(db[~present], pre[1][~present].astype(np.float64)), "absent classes keep their bits (dbeta) " + what
        dg, db = dg - pre[0], db - pre[1]
        ptol = 1e-4
    else:
        assert (dg[~present] == 0).all() and (db[~present] == 0).all(), "absent classes: exact zeros " + what
        ptol = max(tol, 2e-5)
    assert_rows_close(dg[present], dgr[present], ptol, "dgamma " + what)
    assert_rows_close(db[present], dbr[present], ptol, "dbeta " + what)
    if dx0 is not None:
        dxr = dxr + dx0.astype(np.float64)
    assert_channels_close(dx, dxr, tol, "dx " + what)


def _data(mode, rs, n, rps, c, K):
    q = lambda a: half_round(mode, a)
    x, dy = q(rs.randn(n, rps, c) * 1.5 + 0.3), q(rs.randn(n, rps, c))
    gamma = (1.0 + 0.3 * rs.randn(K, c)).astype(np.float32)
    beta = (0.2 * rs.randn(K, c)).astype(np.float32)
    return x, dy, gamma, beta


def _pre(rs, K, c, acc):
    return [rs.randn(K, c).astype(np.float32) for _ in range(2)] if acc else [np.full((K, c), np.nan, np.float32)] * 2


# the smallest magnitude that survives rounding to the storage format (half the smallest subnormal; fp32 and bf16 share an exponent range)
ROUNDS_TO_ZERO = {"f32": 2.0 ** -150, "bf16": 2.0 ** -134, "f16": 2.0 ** -25}


# ---------------------------------------------------------------------------------------------------- sub-sample packing
@pytest.mark.parametrize("c,rps", PACK_CASES)
def test_packed_samples_backward(dev, c, rps):
    """Labelled BN_COLUMN backward with 32 / rps samples to a workgroup (and one short sample each where n or rps does not divide): every
    activation, through rcgan_bn_bwd (mask from y) and rcgan_bn_bwd2 (mask from x), against float64.

    Bit-for-bit rule: the two calls differ only in where the mask comes from -- act'(y), y = storage(act(pre)), against
    act'(storage(pre)) with pre recomputed by the forward's own fp32 sequence.  Both see the same sign unless storage turns a non-zero
    pre (or 0.2 * pre under leaky ReLU) into zero while the other side keeps it, so wherever no |pre| and no 0.2 * |pre| of the case lies
    below the format's round-to-zero bound (ROUNDS_TO_ZERO; pre in float64 from the kernel's own mean and rstd, with a factor 2 for its
    fp32 rounding) dx, dgamma and dbeta of the two calls must be identical.  A case with such an element (none is expected at these
    sizes) is compared within the tolerances only, and says so."""
    ctx, mode = dev
    g = ctx.guard
    K = 10
    for n in pack_ns(rps):
        rs = np.random.RandomState(c * 1000 + rps * 10 + n)
        x, dy, gamma, beta = _data(mode, rs, n, rps, c, K)
        labels = rs.randint(K, size=n)
        present = np.zeros(K, bool)
        present[labels] = True
        r = bn_ref(x, labels, gamma, beta)
        g.clear()
        with g.workspace(ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)):
            for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
                ctx.new_step()
                d = _forward(ctx, x, labels, gamma, beta, K, act)
                what = "c %d rps %d n %d act %d %s" % (c, rps, n, act, mode)
                assert_channels_close(d.yh, act_ref(act, r.pre), TOL[mode], "y " + what)
                ref = bn_ref_bwd(r, dy, mask_of(act, d.yh), K)
                dyd = ctx.upload(dy.reshape(n * rps, c), ctx.act_dtype)
                pre = _pre(rs, K, c, 0)
                outs = {}
                for via in ("y", "beta"):
                    outs[via] = _backward(ctx, d, dyd, via, 0, 0, pre, None)
                    _check_bwd(mode, outs[via], ref, pre, None, 0, present, what + " via " + via)
                mean, rstd = ctx.download(d.mean).astype(np.float64), ctx.download(d.rstd).astype(np.float64)
                inv = rstd * gamma.astype(np.float64)[labels][:, None, :]
                pk = np.abs(x.astype(np.float64) * inv + (beta.astype(np.float64)[labels][:, None, :] - mean * inv))
                if pk[pk > 0].min() * (0.2 if act == ACT_LRELU else 1.0) > 2 * ROUNDS_TO_ZERO[mode]:
                    for k, name in enumerate(("dx", "dgamma", "dbeta")):
                        assert np.array_equal(outs["y"][k], outs["beta"][k]), "%s: mask from y and mask from x differ, %s" % (name, what)
                else:
                    print("underflowing pre-activation: bits not compared, " + what)
            ctx.sync()
            g.check()


# ---------------------------------------------------------------------------------------------------- label edges
def _label_sets(rs, n, K):
    """name -> labels.  K = 17 takes the sets of K = 16 (labels 0 .. 15): the same data on either side of the 16 / 17 boundary."""
    k = min(K, 16)
    single = rs.randint(max(k - 1, 1), size=n)
    if k > 1:
        single[0] = k - 1                                          # class k-1: one sample
    mixed = np.sort(rs.randint(k, size=n))
    return {"last": np.full(n, k - 1), "ends": np.where(rs.rand(n) < 0.5, 0, k - 1), "single": single, "sorted": mixed}


def _label_edges(dev, shape, K, seed, sets=None, runs=((0, 0), (1, 1))):
    ctx, mode = dev
    g = ctx.guard
    n, rps, c = shape
    rs = np.random.RandomState(seed)                               # (the seed does not depend on K: 16 and 17 see the same data)
    x, dy, gamma17, beta17 = _data(mode, rs, n, rps, c, 17)
    gamma, beta = gamma17[:K].copy(), beta17[:K].copy()
    lsets = _label_sets(np.random.RandomState(seed + 1), n, K)
    perm = np.random.RandomState(seed + 2).permutation(n)
    results = {}
    g.clear()
    with g.workspace(ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)):
        for si, (name, labels) in enumerate(lsets.items()):
            if sets is not None and name not in sets:
                continue
            act, via = (ACT_NONE, ACT_RELU, ACT_LRELU)[si % 3], ("y", "beta")[si % 2]
            present = np.zeros(K, bool)
            present[labels] = True
            variants = [("", x, dy, labels)] + ([("interleaved", x[perm], dy[perm], labels[perm])] if name == "sorted" else [])
            for vname, xv, dyv, lv in variants:
                r = bn_ref(xv, lv, gamma, beta)
                ctx.new_step()
                d = _forward(ctx, xv, lv, gamma, beta, K, act)
                what = "%s K %d %s%s act %d via %s %s" % (shape, K, name, vname, act, via, mode)
                assert_channels_close(d.yh, act_ref(act, r.pre), TOL[mode], "y " + what)
                ref = bn_ref_bwd(r, dyv, mask_of(act, d.yh), K)
                dyd = ctx.upload(dyv.reshape(n * rps, c), ctx.act_dtype)
                for acc, acc_dx in runs:
                    prs = np.random.RandomState(seed + 10 * si + acc)
                    pre = _pre(prs, K, c, acc)
                    dx0 = half_round(mode, prs.randn(n, rps, c)) if acc_dx else None
                    got = _backward(ctx, d, dyd, via, acc, acc_dx, pre, dx0)
                    _check_bwd(mode, got, ref, pre, dx0, acc, present, what + " acc %d %d" % (acc, acc_dx))
                    if acc == 0:
                        results[name + vname] = got
            if name == "sorted":
                # the same multiset of (sample, label) pairs in another order: the same sums, up to the summation order
                a, b = results["sorted"], results["sortedinterleaved"]
                tol = max(TOL[mode], 2e-5)
                assert_rows_close(b[1][present], a[1][present], 2 * tol, "dgamma interleaved vs sorted")
                assert_rows_close(b[2][present], a[2][present], 2 * tol, "dbeta interleaved vs sorted")
                assert_channels_close(b[0], a[0][perm], 2 * TOL[mode], "dx interleaved vs sorted")
        ctx.sync()
        g.check()
    return results


@pytest.mark.parametrize("K", LABEL_KS)
@pytest.mark.parametrize("name", sorted(LABEL_SHAPES))
def test_label_edges(dev, name, K):
    """n_labels 1 (with a label vector of zeros), 2, 16 and 17 on the same data: every sample in the last class, only the first and the
    last class, a class with one sample, sorted against interleaved labels; accumulate = 0 into NaN (absent classes exactly 0) and
    accumulate = accumulate_dx = 1 into random buffers (absent classes keep their bits); the activation and the mask's source change
    with the label set."""
    _label_edges(dev, LABEL_SHAPES[name], K, 7 + len(name))


@pytest.mark.parametrize("name", sorted(LABEL_SHAPES))
def test_sixteen_against_seventeen_classes(dev, name):
    """The register / LDS routes (K = 16) and the per-sample route (K = 17) on identical data and labels 0 .. 15 agree within twice the
    tolerance, row by row; row 16 is exactly zero."""
    ctx, mode = dev
    a = _label_edges(dev, LABEL_SHAPES[name], 16, 7 + len(name), sets=("single",), runs=((0, 0),))["single"]
    b = _label_edges(dev, LABEL_SHAPES[name], 17, 7 + len(name), sets=("single",), runs=((0, 0),))["single"]
    tol = max(TOL[mode], 2e-5)
    assert (b[1][16] == 0).all() and (b[2][16] == 0).all()
    assert_rows_close(b[1][:16], a[1], 2 * tol, "dgamma K 17 vs 16")
    assert_rows_close(b[2][:16], a[2], 2 * tol, "dbeta K 17 vs 16")
    assert_channels_close(b[0], a[0], 2 * TOL[mode], "dx K 17 vs 16")


def test_label_edges_tree(dev):
    """BN_TREE, one labelled 4 Mi element case: 16 classes of which only 0, 15 and (one sample) 7 occur; one forward, then accumulate = 0
    into NaN-filled buffers (mask from y) and accumulate = accumulate_dx = 1 into random ones (mask from x)."""
    ctx, mode = dev
    g = ctx.guard
    n, rps, c = TREE_SHAPE
    K = 16
    rs = np.random.RandomState(99)
    x, dy, gamma, beta = _data(mode, rs, n, rps, c, K)
    labels = np.where(rs.rand(n) < 0.5, 0, 15)
    labels[5] = 7
    present = np.zeros(K, bool)
    present[labels] = True
    r = bn_ref(x, labels, gamma, beta)
    g.clear()
    with g.workspace(ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)):
        ctx.new_step()
        d = _forward(ctx, x, labels, gamma, beta, K, ACT_RELU)
        assert_channels_close(d.yh, act_ref(ACT_RELU, r.pre), TOL[mode], "y tree")
        ref = bn_ref_bwd(r, dy, mask_of(ACT_RELU, d.yh), K)
        dyd = ctx.upload(dy.reshape(n * rps, c), ctx.act_dtype)
        pre = _pre(rs, K, c, 0)                                      # into NaN: the thirteen absent classes come out exactly zero
        _check_bwd(mode, _backward(ctx, d, dyd, "y", 0, 0, pre, None), ref, pre, None, 0, present, "tree acc 0 " + mode)
        pre = _pre(rs, K, c, 1)
        dx0 = half_round(mode, rs.randn(n, rps, c))
        _check_bwd(mode, _backward(ctx, d, dyd, "beta", 1, 1, pre, dx0), ref, pre, dx0, 1, present, "tree acc 1 " + mode)
        ctx.sync()
        g.check()


# ---------------------------------------------------------------------------------------------------- grid-stride apply
@pytest.mark.parametrize("name", sorted(STRIDE_CASES))
def test_apply_second_grid_stride(dev, name):
    """Tensors just past 8192 workgroups x 256 items: the scalar, vector and fused apply kernels enter their second grid stride, forward
    and backward (accumulate_dx = 1, so an element visited twice shows as well as one never visited)."""
    ctx, mode = dev
    g = ctx.guard
    n, rps, c = STRIDE_CASES[name]
    K = 10
    rng = np.random.default_rng(len(name))
    q = lambda a: half_round(mode, a)
    x = q(rng.standard_normal((n, rps, c), dtype=np.float32) * 1.5 + 0.3)
    dy = q(rng.standard_normal((n, rps, c), dtype=np.float32))
    dx0 = q(rng.standard_normal((n, rps, c), dtype=np.float32))
    rs = np.random.RandomState(3)
    gamma, beta = (1.0 + 0.3 * rs.randn(K, c)).astype(np.float32), (0.2 * rs.randn(K, c)).astype(np.float32)
    labels = rs.randint(K, size=n)
    present = np.zeros(K, bool)
    present[labels] = True
    r = bn_ref(x, labels, gamma, beta)
    g.clear()
    with g.workspace(ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)):
        ctx.new_step()
        d = _forward(ctx, x, labels, gamma, beta, K, ACT_RELU)
        assert g.unwritten(d.y) == 0
        assert_channels_close(d.yh, act_ref(ACT_RELU, r.pre), TOL[mode], "y " + name)
        del r.pre
        ref = bn_ref_bwd(r, dy, mask_of(ACT_RELU, d.yh), K)
        pre = _pre(rs, K, c, 0)
        got = _backward(ctx, d, ctx.upload(dy.reshape(n * rps, c), ctx.act_dtype), "beta", 0, 1, pre, dx0)
        _check_bwd(mode, got, ref, pre, dx0, 0, present, "stride %s %s" % (name, mode))
        ctx.sync()
        g.check()


# ---------------------------------------------------------------------------------------------------- statistics
def _stats(ctx, x2, eps, moving=None, decay=0.0):
    from rcgan_amd import _lib as L
    rows, c = x2.shape
    xd = ctx.upload(x2, ctx.act_dtype)
    mean, rstd = ctx.empty((c,), L.F32), ctx.empty((c,), L.F32)
    mm = mv = None
    if moving is not None:
        mm, mv = ctx.upload(moving[0], L.F32), ctx.upload(moving[1], L.F32)
    ws, wsb = _ws(ctx)
    ctx.check(ctx.lib.rcgan_bn_stats(ctx.h, rows, c, xd.dtype, _p(xd), eps, _p(mean), _p(rstd), _p(mm), _p(mv), decay, ws, wsb))
    out = [ctx.download(t).astype(np.float64) for t in (mean, rstd)]
    return out + ([ctx.download(mm).astype(np.float64), ctx.download(mv).astype(np.float64)] if moving is not None else []), xd, mean, rstd


def _stats_ref(x2, eps):
    x64 = x2.astype(np.float64)
    mu, var = x64.mean(0), x64.var(0)
    return mu, var, 1.0 / np.sqrt(var + np.float64(np.float32(eps)))


def _stats_case(dev, rows, c, eps):
    """Random channels, channel 0 constant 0 and channel 1 constant 0.75 (where c allows); moving statistics from random positive
    values with decay 0, 0.9, 0.99; then the forward apply: y = beta exactly on the zero channel."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    g = ctx.guard
    rs = np.random.RandomState(rows * 7 + c)
    x = half_round(mode, rs.randn(rows, c) * 1.5 + 0.3)
    x[:, 0] = 0.0
    if c > 2:
        x[:, 1] = 0.75
    mu, var, rstd_ref = _stats_ref(x, eps)
    gamma, beta = (1.0 + 0.3 * rs.randn(1, c)).astype(np.float32), (0.2 * rs.randn(1, c)).astype(np.float32)
    g.clear()
    with g.workspace(ctx.lib.rcgan_bn_workspace_bytes(rows, c)):
        for decay in (0.0, 0.9, 0.99):
            ctx.new_step()
            mv0 = [(0.5 + rs.rand(c)).astype(np.float32) for _ in range(2)]
            (mean, rstd, mm, mv), xd, mean_d, rstd_d = _stats(ctx, x, eps, mv0, decay)
            what = "rows %d c %d eps %g decay %g %s" % (rows, c, eps, decay, mode)
            assert_stats_close(mean, rstd, x, eps, what)
            exact = float(np.float32(1.0 / np.sqrt(np.float64(np.float32(eps)))))
            for ch, v in ((0, 0.0), (1, 0.75))[:2 if c > 2 else 1]:
                assert mean[ch] == v and rstd[ch] == exact, "constant channel %d: mean %r rstd %r (expected %r, %r) %s" % (ch, mean[ch], rstd[ch], v, exact, what)
            # TF's update with Bessel's correction; a single row has no unbiased variance and keeps the biased one (0)
            uvar = var * rows / (rows - 1) if rows > 1 else var
            om = np.float64(np.float32(1.0) - np.float32(decay))
            mm_ref, mv_ref = mv0[0] - (mv0[0] - mu) * om, mv0[1] - (mv0[1] - uvar) * om
            assert np.isfinite(mm).all() and np.isfinite(mv).all(), what
            # 1e-5 as in test_batch_norm, plus what the one-pass fp32 sums may be off by (CHAIN_U above; a one-row batch of fp32 values has
            # fl(x * x) - x * x for a variance, not zero)
            x64 = x.astype(np.float64)
            dm = CHAIN_U * np.abs(x64).mean(0)
            dv = CHAIN_U * ((x64 * x64).mean(0) + 2 * np.abs(mu) * np.abs(x64).mean(0)) * (rows / (rows - 1.0) if rows > 1 else 1.0)
            assert (np.abs(mm - mm_ref) <= 1e-5 * np.abs(mm_ref).max() + om * dm).all(), "moving mean " + what
            assert (np.abs(mv - mv_ref) <= 1e-5 * np.abs(mv_ref).max() + om * dv).all(), "moving variance " + what
        y = ctx.empty((rows, c), ctx.act_dtype)
        gd, bd = ctx.upload(gamma, L.F32), ctx.upload(beta, L.F32)
        ws, wsb = _ws(ctx)
        ctx.check(ctx.lib.rcgan_bn_apply_fwd(ctx.h, 1, rows, c, 1, xd.dtype, _p(xd), None, _p(gd), _p(bd), _p(mean_d), _p(rstd_d), ACT_NONE, _p(y), ws, wsb))
        yh = ctx.download(y).astype(np.float64)
        assert np.array_equal(yh[:, 0], np.full(rows, half_round(mode, beta[0, :1])[0], np.float64)), "y = beta on the zero channel"
        # every channel: y = x * inv + (beta - mean * inv) as tf.nn.batch_normalization has it, inv = rstd * gamma.  Where the spread is
        # small beside the mean (the 0.75 channel, every channel of a one-row batch, some of a two-row batch) x * inv and mean * inv are large
        # and cancel: two fp32 roundings at THEIR size, which is therefore part of the scale; the kernel's own rstd stands in the reference
        # (its error has its own check above)
        inv = rstd * gamma[0].astype(np.float64)
        yr = (x.astype(np.float64) - mu) * inv + beta[0]
        assert_channels_close(yh, yr, TOL[mode], "y rows %d c %d %s" % (rows, c, mode), extra=np.abs(mu * inv))
        ctx.sync()
        g.check()


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("c", sorted(STATS_ROWS))
def test_stats_rows(dev, c, eps):
    for rows in STATS_ROWS[c]:
        _stats_case(dev, rows, c, eps)


def test_stats_tree(dev):
    _stats_case(dev, STATS_TREE[0], STATS_TREE[1], 1e-5)


OFFSET_RATIOS = []


@pytest.mark.parametrize("rows,c", [(4096, 64), (4096, 24), (4096, 20), STATS_TREE])
def test_stats_offset_channels(dev, rows, c):
    """x = m + randn with m / std = 8 (first half of the channels) and 64 (second half).  The bound is not invented: the same moments
    computed one-pass in float32 with numpy (np.sum of float32 x and x * x, the variance from them in float64) have an error against
    float64 that any one-pass fp32 scheme has on this input; the kernel may have 4 times that (another summation order) plus the
    project's fp32 tolerance, on mean and on rstd, per group of channels."""
    ctx, mode = dev
    g = ctx.guard
    rs = np.random.RandomState(rows + c)
    m = np.where(np.arange(c) < c // 2, 8.0, 64.0)
    x = half_round(mode, rs.randn(rows, c) + m)
    mu, var, rstd_ref = _stats_ref(x, 1e-5)
    s1 = np.sum(x, axis=0, dtype=np.float32).astype(np.float64)
    s2 = np.sum(x * x, axis=0, dtype=np.float32).astype(np.float64)
    mu_np = s1 / rows
    rstd_np = 1.0 / np.sqrt(np.maximum(s2 / rows - mu_np * mu_np, 0.0) + np.float64(np.float32(1e-5)))
    g.clear()
    with g.workspace(ctx.lib.rcgan_bn_workspace_bytes(rows, c)):
        ctx.new_step()
        (mean, rstd), _, _, _ = _stats(ctx, x, 1e-5)
        ctx.sync()
        g.check()
    for ratio, sl in ((8, slice(0, c // 2)), (64, slice(c // 2, c))):
        for name, got, ref, onepass in (("mean", mean, mu, mu_np), ("rstd", rstd, rstd_ref, rstd_np)):
            e_k, e_np = np.abs(got[sl] - ref[sl]).max(), np.abs(onepass[sl] - ref[sl]).max()
            bound = 4 * e_np + TOL["f32"] * np.abs(ref[sl]).max()
            line = "offset channels rows %d c %d %s m/std %d %s: kernel err %.3e, numpy one-pass fp32 err %.3e, ratio %.3g, bound %.3e" % (
                rows, c, mode, ratio, name, e_k, e_np, e_k / e_np if e_np else float("inf") if e_k else 0.0, bound)
            print(line)
            OFFSET_RATIOS.append(line)
            assert e_k <= bound, line


# ---------------------------------------------------------------------------------------------------- segmented forward
def _segments(dev, nseg, shape, labels, K, seed, const_channel=False, operand_scale=False):
    """rcgan_bn_fwd_segments with y, then statistics only + rcgan_bn_apply_segments: per segment against float64, per channel."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    g = ctx.guard
    n, rps, c = shape
    rs = np.random.RandomState(seed)
    x = half_round(mode, rs.randn(nseg, n, rps, c) * 1.3 + rs.randn(nseg, 1, 1, 1))
    if const_channel:
        x[..., 0] = 0.75
    gamma, beta = (1 + 0.3 * rs.randn(K, c)).astype(np.float32), (0.2 * rs.randn(K, c)).astype(np.float32)
    g.clear()
    with g.workspace(nseg * ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)):
        ctx.new_step()
        xd, lab, gd, bd = ctx.upload(x.reshape(-1, c), ctx.act_dtype), ctx.upload(labels.astype(np.int32)), ctx.upload(gamma, L.F32), ctx.upload(beta, L.F32)
        ws, wsb = _ws(ctx)
        mean, rstd, y = ctx.empty((nseg, c), L.F32), ctx.empty((nseg, c), L.F32), ctx.empty((nseg * n * rps, c), ctx.act_dtype)
        ctx.check(ctx.lib.rcgan_bn_fwd_segments(ctx.h, nseg, n, rps, c, K, xd.dtype, _p(xd), _p(lab), _p(gd), _p(bd), 1e-5, ACT_RELU, _p(mean), _p(rstd), _p(y),
                                                ws, wsb))
        assert g.unwritten(y) == 0 and g.unwritten(mean) == 0 and g.unwritten(rstd) == 0
        yh = ctx.download(y).astype(np.float64).reshape(nseg, n, rps, c)
        mh, rh = ctx.download(mean).astype(np.float64), ctx.download(rstd).astype(np.float64)
        for k in range(nseg):
            r = bn_ref(x[k], labels[k * n:(k + 1) * n], gamma, beta)
            assert_stats_close(mh[k], rh[k], x[k].reshape(-1, c), 1e-5, "segment %d" % k)
            if const_channel:
                assert mh[k, 0] == 0.75 and rh[k, 0] == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))), "segment %d constant channel" % k
            if operand_scale:      # (as in _stats_case: the kernel's rstd in the reference, the size of mean * inv in the scale)
                lab_k = labels[k * n:(k + 1) * n]
                inv = rh[k] * gamma.astype(np.float64)[lab_k][:, None, :]
                pre_k = (x[k].astype(np.float64) - r.mu) * inv + beta.astype(np.float64)[lab_k][:, None, :]
                assert_channels_close(yh[k], act_ref(ACT_RELU, pre_k), TOL[mode], "segment %d y" % k, extra=np.abs(r.mu * inv).max((0, 1)))
            else:
                assert_channels_close(yh[k], act_ref(ACT_RELU, r.pre), TOL[mode], "segment %d y" % k)
        mean2, rstd2, y2 = ctx.empty((nseg, c), L.F32), ctx.empty((nseg, c), L.F32), ctx.empty((nseg * n * rps, c), ctx.act_dtype)
        ctx.check(ctx.lib.rcgan_bn_fwd_segments(ctx.h, nseg, n, rps, c, K, xd.dtype, _p(xd), _p(lab), _p(gd), _p(bd), 1e-5, ACT_RELU, _p(mean2), _p(rstd2), None,
                                                ws, wsb))
        assert np.array_equal(ctx.download(mean2), ctx.download(mean)) and np.array_equal(ctx.download(rstd2), ctx.download(rstd))
        ctx.check(ctx.lib.rcgan_bn_apply_segments(ctx.h, nseg, n, rps, c, K, xd.dtype, _p(xd), _p(lab), _p(gd), _p(bd), _p(mean2), _p(rstd2), ACT_RELU, _p(y2),
                                                  ws, wsb))
        assert np.array_equal(ctx.download(y2), ctx.download(y)), "apply_segments differs from the one-call output"
        ctx.sync()
        g.check()


def test_segments_all_counter_lines(dev):
    """8 segments x 2048 channels = 256 (segment, column block) pairs: the last count that is still one launch."""
    nseg, shape = SEGMENT_LINES_CASE
    _segments(dev, nseg, shape, np.random.RandomState(1).randint(10, size=nseg * shape[0]), 10, 41)


def test_one_segment(dev):
    """nseg = 1: rcgan_bn_apply_segments is the plain apply."""
    _segments(dev, 1, (6, 16, 64), np.random.RandomState(2).randint(10, size=6), 10, 42)


def test_segments_with_absent_classes(dev):
    """Segment 0 holds class 3 only, segment 1 classes 0 and 9, segment 2 all of them."""
    n = 12
    rs = np.random.RandomState(3)
    labels = np.concatenate([np.full(n, 3), np.where(rs.rand(n) < 0.5, 0, 9), rs.randint(10, size=n)])
    _segments(dev, 3, (n, 16, 64), labels, 10, 43)


def test_segment_statistics_edges(dev):
    """Segments of 1, 2 and 513 rows with a constant channel (statistics per segment, biased variance)."""
    for rows in (1, 2, 513):
        _segments(dev, 3, (1, rows, 64), np.random.RandomState(rows).randint(10, size=3), 10, 44 + rows, const_channel=True, operand_scale=True)


# ---------------------------------------------------------------------------------------------------- workspace contract
def test_query_formulas(dev):
    ctx, _ = dev
    for rows, c, K in QUERY_SHAPES:
        assert ctx.lib.rcgan_bn_workspace_bytes_labels(rows, c, K) == query_bytes(rows, c, K), (rows, c, K)
        assert ctx.lib.rcgan_bn_workspace_bytes(rows, c) == query_bytes(rows, c), (rows, c)


def test_backward_past_the_query_is_refused(dev):
    """The first n at which a labelled backward needs more than the query function returns (include/rcgan_hip.h, rcgan_bn_bwd): with the
    query's byte count the call returns RCGAN_EWORKSPACE_TOO_SMALL and writes nothing -- outputs and workspace still hold the fill;
    one sample fewer, and the same call goes through."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    g = ctx.guard
    route, rps, c, K = CONTRACT_CASE
    for n, expect in ((FIRST_EXCEED[CONTRACT_CASE], EWORKSPACE_TOO_SMALL), (FIRST_EXCEED[CONTRACT_CASE] - 1, 0)):
        rs = np.random.RandomState(n)
        x, dy, gamma, beta = _data(mode, rs, n, rps, c, K)
        labels = rs.randint(K, size=n)
        g.clear()
        with g.workspace(ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K)) as frame:
            ctx.new_step()
            d = _forward(ctx, x, labels, gamma, beta, K, ACT_RELU)
            g.refill_workspace()
            dyd = ctx.upload(dy.reshape(n * rps, c), ctx.act_dtype)
            dx, dg, db = ctx.empty((n * rps, c), ctx.act_dtype), ctx.empty((K, c), L.F32), ctx.empty((K, c), L.F32)
            ws, wsb = _ws(ctx)
            rc = ctx.lib.rcgan_bn_bwd(ctx.h, n, rps, c, K, d.x.dtype, _p(d.x), _p(d.y), _p(dyd), _p(d.lab), _p(d.g), _p(d.mean), _p(d.rstd), ACT_RELU,
                                      _p(dx), 0, _p(dg), _p(db), 0, ws, wsb)
            ctx.sync()
            assert rc == expect, (n, rc, ctx.lib.rcgan_last_error(ctx.h))
            if expect:
                assert g.unwritten(dx) == dx.size and g.unwritten(dg) == dg.size and g.unwritten(db) == db.size, "a refused call wrote an output"
                assert bool((frame.raw == 0xFF).all()), "a refused call wrote the workspace"
            else:
                assert g.unwritten(dx) == 0 and g.unwritten(dg) == 0 and g.unwritten(db) == 0
            g.check()
