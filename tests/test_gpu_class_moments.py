"""rcgan_class_moments_accum (csrc/moments.hip) against float64 numpy on the same fp32 inputs.

The bound is derived, not tuned: a product of two fp32 values is exact in fp64, an entry is a sum of at most n such products added
one after the other, so |err| <= n 2^-52 sum|x_i x_j| over the class's rows (the reference's own summation error included), and
the same with sum|x_i| -- times 4 -- for the sums.  Counts and the rejected counter are exact.  The state sits between two sentinel
margins that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frechet_ref as FRF
from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

MARGIN, SENTINEL = 256, 0xA5
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 26)
    yield c
    c.close()


class State:
    """A zeroed state for (d, K) between two sentinel margins."""

    def __init__(self, ctx, d, K):
        self.d, self.K = d, K
        self.nbytes = ctx.lib.rcgan_class_moments_bytes(d, K)
        assert self.nbytes == 8 * (K + K * d + K * d * d + 1)
        self.raw = torch.full((MARGIN + self.nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        self.raw[MARGIN:MARGIN + self.nbytes] = 0
        self.ptr = C.c_void_p(self.raw.data_ptr() + MARGIN)
        torch.cuda.synchronize()

    def get(self):
        """-> (count, sum, sumsq, rejected) float64 numpy; the margins are checked."""
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:MARGIN] == SENTINEL).all() and (raw[MARGIN + self.nbytes:] == SENTINEL).all(), "a sentinel margin was overwritten"
        a = raw[MARGIN:MARGIN + self.nbytes].view(np.float64)
        d, K = self.d, self.K
        return a[:K].copy(), a[K:K + K * d].reshape(K, d).copy(), a[K + K * d:-1].reshape(K, d, d).copy(), a[-1]


def _accum(ctx, st, x, labels):
    """One call on host arrays (uploaded first).  -> the device tensors, kept alive by the caller."""
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(ctx.device)
    ld = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(ctx.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcgan_class_moments_accum(ctx.h, x.shape[0], x.shape[1], st.K, C.c_void_p(xd.data_ptr()),
                                                C.c_void_p(ld.data_ptr()) if ld is not None else None, st.ptr))
    ctx.sync()
    return xd, ld


def _check(got, x, labels, K, what=""):
    """got = State.get() after accumulating exactly the rows of x (in any number of calls)."""
    n = x.shape[0]
    count, s, ss, rejected, sa, ssa = FRF.class_sums(x, labels, K)
    assert np.array_equal(got[0], count), what
    assert got[3] == rejected, (what, got[3], rejected)
    assert (np.abs(got[1] - s) <= 4 * n * EPS * sa).all(), (what, np.abs(got[1] - s).max())
    assert (np.abs(got[2] - ss) <= n * EPS * ssa).all(), (what, np.abs(got[2] - ss).max())


def _data(seed, n, d, K, labelled=True):
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, d) * rs.uniform(0.2, 3.0, d) + rs.randn(d)).astype(np.float32)
    return x, (rs.randint(K, size=n).astype(np.int32) if labelled else None)


# every n of {1, 63, 257, 1000}, d of {1, 3, 64, 67, 256} and K of {1 (labels NULL), 2, 10, 17, 1024} at least once, and the two
# production points
SHAPES = [(1, 1, 1), (63, 3, 2), (257, 67, 17), (63, 256, 2), (257, 3, 1024), (1000, 64, 1), (1000, 64, 10), (1000, 64, 100), (1, 64, 10)]


@pytest.mark.parametrize("n,d,K", SHAPES)
def test_one_call_matches_float64_within_the_derived_bound(ctx, n, d, K):
    x, labels = _data(n + d + K, n, d, K, labelled=K > 1)
    st = State(ctx, d, K)
    _accum(ctx, st, x, labels)
    got = st.get()
    _check(got, x, labels, K)
    assert got[0].sum() == n
    assert np.array_equal(got[2], got[2].transpose(0, 2, 1))          # x_i x_j and x_j x_i: the same products in the same order


def test_all_rows_in_one_class_and_an_absent_class_stays_zero_over_a_later_call(ctx):
    n, d, K = 257, 67, 17
    x, _ = _data(1, n, d, K)
    st = State(ctx, d, K)
    labels = np.full(n, 5, np.int32)
    _accum(ctx, st, x, labels)
    first = st.get()
    _check(first, x, labels, K)
    assert first[0][5] == n and first[0].sum() == n
    others = [k for k in range(K) if k != 5]
    assert not first[1][others].any() and not first[2][others].any()
    # a later call that has class 3 and 5 but none of the others: class 9 (say) is still all zeros, class 5 grew
    x2, _ = _data(2, 63, d, K)
    labels2 = np.where(np.arange(63) % 2 == 0, 3, 5).astype(np.int32)
    _accum(ctx, st, x2, labels2)
    second = st.get()
    _check(second, np.concatenate([x, x2]), np.concatenate([labels, labels2]), K)
    rest = [k for k in range(K) if k not in (3, 5)]
    assert not second[0][rest].any() and not second[1][rest].any() and not second[2][rest].any()


def test_labels_outside_the_classes_are_counted_and_written_nowhere(ctx):
    n, d, K = 1000, 64, 10
    x, labels = _data(3, n, d, K)
    bad = np.random.RandomState(4).choice(n, 37, replace=False)
    labels[bad[:20]], labels[bad[20:]] = -1, K
    labels[bad[0]], labels[bad[1]] = -(2 ** 31), 2 ** 31 - 1
    st = State(ctx, d, K)
    _accum(ctx, st, x, labels)
    got = st.get()                         # (checks the margins)
    assert got[3] == 37 and got[0].sum() == n - 37
    _check(got, x, labels, K)              # (the reference sums leave those rows out of every class)


def test_three_calls_on_thirds_and_one_call_on_the_whole_are_both_within_the_bound(ctx):
    n, d, K = 1000, 64, 10
    x, labels = _data(5, n, d, K)
    whole, thirds = State(ctx, d, K), State(ctx, d, K)
    _accum(ctx, whole, x, labels)
    for lo, hi in ((0, 333), (333, 667), (667, n)):
        _accum(ctx, thirds, x[lo:hi], labels[lo:hi])
    _check(whole.get(), x, labels, K, "one call")
    _check(thirds.get(), x, labels, K, "three calls")


def test_the_same_call_twice_from_zeroed_state_gives_the_same_bits(ctx):
    n, d, K = 1000, 64, 100
    x, labels = _data(6, n, d, K)
    a, b = State(ctx, d, K), State(ctx, d, K)
    _accum(ctx, a, x, labels)
    _accum(ctx, b, x, labels)
    torch.cuda.synchronize()
    assert torch.equal(a.raw, b.raw)


def test_a_captured_call_replayed_twice_equals_two_eager_calls_bit_for_bit(ctx):
    n, d, K = 257, 64, 10
    x, labels = _data(7, n, d, K)
    eager, replay = State(ctx, d, K), State(ctx, d, K)
    xd, ld = _accum(ctx, eager, x, labels)
    _accum(ctx, eager, x, labels)
    call = lambda: ctx.check(ctx.lib.rcgan_class_moments_accum(ctx.h, n, d, K, C.c_void_p(xd.data_ptr()), C.c_void_p(ld.data_ptr()), replay.ptr))
    ctx.graph_begin()
    try:
        call()
    except BaseException:
        ctx.graph_abort()
        raise
    gid = ctx.graph_end()
    try:
        ctx.sync()
        assert not replay.get()[0].any()               # capturing ran nothing
        ctx.graph_launch(gid)
        ctx.graph_launch(gid)
        ctx.sync()
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))
    torch.cuda.synchronize()
    assert torch.equal(eager.raw, replay.raw)
    assert replay.get()[0].sum() == 2 * n


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(ctx):
    from rcgan_amd import _lib as L
    st = State(ctx, 4, 2)
    x = torch.zeros(8, 4, device=ctx.device)
    lab = torch.zeros(8, dtype=torch.int32, device=ctx.device)
    torch.cuda.synchronize()
    f = ctx.lib.rcgan_class_moments_accum
    p = lambda t: C.c_void_p(t.data_ptr())
    for args in ((0, 4, 2, p(x), p(lab), st.ptr), (8, 0, 2, p(x), p(lab), st.ptr), (8, 257, 2, p(x), p(lab), st.ptr),
                 (8, 4, 0, p(x), p(lab), st.ptr), (8, 4, 1025, p(x), p(lab), st.ptr), (8, 4, 2, p(x), None, st.ptr),
                 (8, 4, 2, None, p(lab), st.ptr), (8, 4, 2, p(x), p(lab), None)):
        assert f(ctx.h, *args) == L.EINVALID_ARG, args
        assert b"rcgan_class_moments_accum" in ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    assert not any(np.any(a) for a in st.get())


def test_fp64_accumulation_keeps_a_small_covariance_on_a_large_mean(ctx):
    """The case an fp32 accumulator fails: features 100 + 0.1 N(0, 1).  sum x x^T is ~1e7 per entry and the covariance ~1e-2: the
    difference loses 9 digits, which fp64 has to spare (the derived bound gives ~1e-10 relative) and fp32 does not (percent)."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import frechet as FR
    n, d = 1000, 64
    x = (100.0 + 0.1 * np.random.RandomState(8).randn(n, d)).astype(np.float32)
    st = State(ctx, d, 1)
    _accum(ctx, st, x, None)
    got = st.get()
    mom = FR.moments_from_sums(got[0], got[1], got[2], got[3])
    m, c = FRF.moments(x)
    assert np.abs(mom.cov[0] - c).max() <= 1e-8 * np.abs(c).max(), np.abs(mom.cov[0] - c).max() / np.abs(c).max()
    assert np.abs(mom.pooled[2] - c).max() <= 1e-8 * np.abs(c).max()
    assert np.abs(mom.mean[0] - m).max() <= 1e-12 * np.abs(m).max()


def test_the_wrapper_accumulates_downloads_and_forms_the_pooled_moments(ctx):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import frechet as FR
    n, d, K = 257, 64, 10
    x, labels = _data(9, n, d, K)
    labels[:3] = (-1, K, K + 5)
    ctx.new_step()
    mom = FR.ClassMoments(ctx, d, K)
    mom.add(ctx.upload(x[:100], ctx.act_dtype), ctx.upload(labels[:100]))
    mom.add(ctx.upload(x[100:], ctx.act_dtype), ctx.upload(labels[100:]))
    got, want = mom.download(), FR.moments_of(x, labels, K)
    assert np.array_equal(got.count, want.count) and got.rejected == want.rejected == 3 and got.pooled[0] == n - 3
    scale = np.abs(want.cov).max()
    assert np.abs(got.mean - want.mean).max() <= 1e-12 and np.abs(got.cov - want.cov).max() <= 1e-10 * scale
    assert np.abs(got.pooled[2] - want.pooled[2]).max() <= 1e-10 * scale
    one = FR.ClassMoments(ctx, d, 1)
    one.add(ctx.upload(x, ctx.act_dtype))
    assert one.download().count[0] == n
    with pytest.raises(ValueError):
        FR.ClassMoments(ctx, 257, 1)
    with pytest.raises(ValueError):
        mom.add(ctx.upload(x[:, :63], ctx.act_dtype), ctx.upload(labels))
