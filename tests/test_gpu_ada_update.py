"""rcgan_ada_update (csrc/augment.hip) against the float32 restatement of its definition (tests/ada_ref.update): the whole float[8]
state is compared EXACTLY after every call -- the sum of signs is a sum of small integers, and every other operation is one fp32
operation in a stated order, so there is no tolerance to choose.

State, logits and labels live between guard margins (tests/guard.py): the margins must be intact after every call.

The out-of-range rule the definition chose -- a row whose label is outside [0, ld) counts as ZERO and nothing is read for it -- is
pinned here: such rows' logits are NaN-free poison (+-inf in every column), which would move the sum if any column were read.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ada_ref as A
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

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


def special_scores(n, seed):
    """n scores: +-0, NaN, +-inf, denormals of both signs, then random ones of both signs."""
    rs = np.random.RandomState(seed)
    s = rs.randn(n).astype(np.float32)
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)
    k = min(n, len(sp))
    s[rs.permutation(n)[:k]] = sp[:k]
    return s


def call(ctx, g, st, logits, labels, target, images, interval):
    from rcgan_amd import _lib as L
    n, ld = logits.shape
    lg = ctx.upload(logits, dtype=L.F32)
    lab = ctx.upload(np.asarray(labels, np.int32)) if labels is not None else None
    ctx.check(ctx.lib.rcgan_ada_update(ctx.h, n, C.c_void_p(lg.ptr), ld, C.c_void_p(lab.ptr) if lab is not None else None, C.c_void_p(st.ptr),
                                       target, images, interval))
    ctx.sync()
    g.check()
    return ctx.download(st)


def same(got, want, what):
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), np.asarray(want, np.float32).view(np.int32)), (what, got, want)


@pytest.mark.parametrize("n", [1, 64, 257, 1000])
@pytest.mark.parametrize("interval", [1, 4])
def test_single_column_without_labels(n, interval):
    from rcgan_amd import _lib as L
    ctx, g = env()
    target, images = 0.1, 3.0 * n * interval
    ref = A.new_state(0.5)
    st = ctx.upload(ref, dtype=L.F32)
    ps = []
    for k in range(1, 6):
        lg = special_scores(n, 10 * n + k).reshape(n, 1)
        ref = A.update(ref, lg, None, target, images, interval)
        same(call(ctx, g, st, lg, None, target, images, interval), ref, "call %d" % k)
        ps.append(float(ref[0]))
    if interval == 4:
        # calls 3, 4 and 5: no change of p, then the change and the reset, then a fresh accumulation
        assert ps[2] == ps[1] == 0.5 and ref[5] == 1 and ref[3] == 1 and ref[2] == n
        if n > 1:
            assert ps[3] != ps[2] and ps[4] == ps[3]
    else:
        assert ref[5] == 5 and ref[1] == ref[2] == ref[3] == 0


@pytest.mark.parametrize("n", [1, 64, 257, 1000])
def test_ten_columns_with_labels_and_the_out_of_range_rule(n):
    from rcgan_amd import _lib as L
    ctx, g = env()
    ld, interval, target, images = 10, 2, -0.2, 5.0 * n
    rs = np.random.RandomState(n)
    ref = A.new_state(0.3)
    st = ctx.upload(ref, dtype=L.F32)
    for k in range(1, 5):
        lab = rs.randint(0, ld, size=n).astype(np.int32)
        lab[0] = 0 if k % 2 else 9
        lg = rs.randn(n, ld).astype(np.float32)
        lg[np.arange(n), lab] = special_scores(n, 7 * n + k)
        if n >= 64:
            # labels outside [0, ld): the row counts as zero whatever it holds (every column poisoned with +-inf)
            bad = np.array([1, 5, 17, n - 1])
            lab[bad] = [-1, ld, 2 ** 31 - 1, -2 ** 31]
            lg[bad] = np.where(np.arange(ld) % 2, np.inf, -np.inf).astype(np.float32)
            lab[[2, 3]] = [0, 9]
        assert (A.scores(lg, lab)[lab < 0] == 0).all()
        ref = A.update(ref, lg, lab, target, images, interval)
        same(call(ctx, g, st, lg, lab, target, images, interval), ref, "call %d" % k)
    assert ref[5] == 2


def test_out_of_range_rows_count_as_images_and_as_zero():
    from rcgan_amd import _lib as L
    ctx, g = env()
    lg = np.full((4, 3), np.inf, np.float32)
    st = ctx.upload(A.new_state(0.5), dtype=L.F32)
    got = call(ctx, g, st, lg, [3, -1, 0, 2], 0.25, 16.0, 1)
    same(got, A.update(A.new_state(0.5), lg, [3, -1, 0, 2], 0.25, 16.0, 1), "state")
    assert got[4] == 0.5 and got[0] == 0.75                       # r = 2 / 4 (not 2 / 2): above the target, p += 4 / 16


def test_clamping_at_both_ends_and_r_equal_to_target():
    from rcgan_amd import _lib as L
    ctx, g = env()
    up, down = np.ones((8, 1), np.float32), -np.ones((8, 1), np.float32)
    ref = A.new_state(0.9)
    st = ctx.upload(ref, dtype=L.F32)
    for k, lg in enumerate([up] * 3 + [down] * 6):
        ref = A.update(ref, lg, None, 0.6, 32.0, 1)
        same(call(ctx, g, st, lg, None, 0.6, 32.0, 1), ref, "call %d" % k)
        if k == 2:
            assert ref[0] == 1.0
    assert ref[0] == 0.0 and ref[5] == 9
    # r == target exactly: p stays where it is, the update is still counted
    lg = np.array([[1.0], [1.0], [1.0], [-1.0]], np.float32)
    ref = A.new_state(0.25)
    st = ctx.upload(ref, dtype=L.F32)
    ref = A.update(ref, lg, None, 0.5, 16.0, 1)
    same(call(ctx, g, st, lg, None, 0.5, 16.0, 1), ref, "r == target")
    assert ref[0] == np.float32(0.25) and ref[4] == np.float32(0.5) and ref[5] == 1
