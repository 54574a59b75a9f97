"""rcgan_poly3_rowsum (csrc/ksum.hip) against brute-force float64 numpy (tests/kid_ref.py) on the same fp32 inputs.

Exact cases: integer features in [-4, 4], gamma = 2^-6, coef0 = 1.  An inner product is an integer of magnitude <= 16 d <= 4096, exact
in fp32 in any order; t = dot / 64 + 1 is a multiple of 2^-6 with |t| <= 65, so t^3 is an integer multiple of 2^-18 below 2^19 and a
sum of up to 257 of them stays below 2^28: in units of 2^-18 every partial sum is an integer below 2^46, exact in fp64 in ANY order.
Row sums must EQUAL the reference.  Sizes: 1, 2, one below / at / one above every tile edge of the kernel as built -- 32 (one
wavefront's reference rows, one MFMA column block), 64 (a workgroup's query tile), 128 (a workgroup's staged reference tile) -- then
130 and 257; d of {1, 2, 3, 64, 67, 255, 256} (odd, a 16-byte row, one chunk, across a chunk, the bound).

Real-valued cases: the bound is derived, not tuned.  The fp32 inner product of d terms, fused or not, in any order, has
|dot_c - dot| <= E = g_d sum_i |q_i r_i| with g_d = d u / (1 - d u), u = 2^-24.  Then t_c = gamma dot_c + coef0 in fp64 is within
gamma E (+ roundings) of t, |t_c^3 - t^3| <= 3 (|t| + gamma E)^2 gamma E, the fp64 operations on one term cost at most 8 2^-53 |t|^3
and a sum of n terms in any order n 2^-53 sum_j |t_j|^3:
    |rowsum - ref| <= sum_j [ 3 (|t| + gamma E)^2 gamma E + 8 2^-53 |t|^3 ] + n 2^-53 sum_j |t|^3.
Before it is used, the bound of every row is asserted to be below the smallest single |k(q_i, r_j)| of that row, so one dropped or
doubled pair cannot hide in it.  The same sets shifted by +100 in every coordinate must meet the same bound.

Every output sits between two sentinel margins that must come back untouched, and starts out filled with the sentinel: a row the
kernel did not write is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kid_ref as KR
from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

MARGIN, SENTINEL = 256, 0xA5
UNWRITTEN_I64 = np.frombuffer(bytes([SENTINEL] * 8), np.int64)[0]
GAMMA_EXACT, COEF0 = 2.0 ** -6, 1.0
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257]
DS = [1, 2, 3, 64, 67, 255, 256]


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 26)
    yield c
    c.close()


class Out:
    """n fp64 outputs between two sentinel margins, themselves filled with the sentinel."""

    def __init__(self, ctx, n):
        self.n = n
        self.raw = torch.full((MARGIN + 8 * n + MARGIN,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        assert (self.raw.data_ptr() + MARGIN) % 8 == 0
        self.ptr = C.c_void_p(self.raw.data_ptr() + MARGIN)

    def get(self):
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:MARGIN] == SENTINEL).all() and (raw[MARGIN + 8 * self.n:] == SENTINEL).all(), "a sentinel margin was overwritten"
        return raw[MARGIN:MARGIN + 8 * self.n].view(np.float64).copy()


def _dev(ctx, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(ctx.device)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run(ctx, q, q_off, r, r_off, gamma, coef0, exclude=False):
    qd, rd = _dev(ctx, q, np.float32), _dev(ctx, r, np.float32)
    qo, ro = _dev(ctx, q_off, np.int32), _dev(ctx, r_off, np.int32)
    out = Out(ctx, len(q))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcgan_poly3_rowsum(ctx.h, q.shape[0], r.shape[0], q.shape[1], len(q_off) - 1, _p(qd), _p(qo), _p(rd), _p(ro),
                                         gamma, coef0, 1 if exclude else 0, out.ptr))
    ctx.sync()
    return out.get()


def _ints(seed, n, d):
    return np.random.default_rng(seed).integers(-4, 5, size=(n, d)).astype(np.float32)


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _unwritten(v):
    return v.view(np.int64) == UNWRITTEN_I64


# ------------------------------------------------------------------------------------------------------------------- exact
# every size as the query count and as the reference count, every d with several of them, d = 256 with the largest sizes
ONE = sorted(set([(e, SIZES[(i + 5) % 13], DS[i % 7]) for i, e in enumerate(SIZES)] +
                 [(SIZES[(i + 3) % 13], e, DS[(i + 2) % 7]) for i, e in enumerate(SIZES)] +
                 [(257, 257, 256), (130, 257, 64), (257, 130, 67), (129, 129, 255), (65, 33, 1), (64, 128, 64), (1, 1, 1), (2, 2, 2)]))


@pytest.mark.parametrize("nq,nr,d", ONE)
def test_row_sums_of_integer_features_equal_the_reference(ctx, nq, nr, d):
    q, r = _ints(nq + d, nq, d), _ints(nr + d + 1000, nr, d)
    want, written = KR.rowsum_segmented(q, _off([nq]), r, _off([nr]), GAMMA_EXACT, COEF0)
    got = run(ctx, q, _off([nq]), r, _off([nr]), GAMMA_EXACT, COEF0)
    assert written.all() and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # exclude_same_row between DIFFERENT tensors still means "global row index equal"
    want_x, _ = KR.rowsum_segmented(q, _off([nq]), r, _off([nr]), GAMMA_EXACT, COEF0, True)
    got_x = run(ctx, q, _off([nq]), r, _off([nr]), GAMMA_EXACT, COEF0, exclude=True)
    assert np.array_equal(got_x, want_x), np.flatnonzero(got_x != want_x)[:10]


@pytest.mark.parametrize("n,d", sorted(set([(e, DS[(i + 4) % 7]) for i, e in enumerate(SIZES)] + [(257, 256), (130, 64), (128, 67), (64, 255)])))
def test_a_set_against_itself_without_the_diagonal_is_the_full_sum_minus_the_diagonal(ctx, n, d):
    x = _ints(3 * n + d, n, d)
    off = _off([n])
    full = run(ctx, x, off, x, off, GAMMA_EXACT, COEF0)
    without = run(ctx, x, off, x, off, GAMMA_EXACT, COEF0, exclude=True)
    diag = np.diag(KR.kernel(x, x, GAMMA_EXACT, COEF0))
    assert np.array_equal(full, KR.rowsum_segmented(x, off, x, off, GAMMA_EXACT, COEF0)[0])
    assert np.array_equal(without, KR.rowsum_segmented(x, off, x, off, GAMMA_EXACT, COEF0, True)[0])
    assert np.array_equal(without, full - diag)                     # (exact: every value is a small multiple of 2^-18)
    if n == 1:
        assert without[0] == 0.0


# (d, query sizes, reference sizes): an empty segment on either side, one-row segments, sizes straddling 32 / 64 / 128
SEGMENTED = [(64, [3, 0, 10, 64, 1, 7, 40, 5, 129], [0, 1, 5, 6, 70, 0, 130, 45, 33]),
             (3, [100, 1, 65, 27, 64], [1, 2, 0, 90, 37]),
             (67, [60, 70, 0, 2, 125], [16, 17, 1, 0, 96]),
             (256, [0, 65, 1, 9, 2, 180], [5, 6, 60, 0, 1, 58])]


@pytest.mark.parametrize("d,q_sizes,r_sizes", SEGMENTED)
def test_row_sums_per_segment_equal_the_reference(ctx, d, q_sizes, r_sizes):
    nq, nr = sum(q_sizes), sum(r_sizes)
    trailing = 7                                                    # rows after the last segment: in no segment, not written
    q, r = _ints(nq + d, nq + trailing, d), _ints(nr + d + 1000, nr + trailing, d)
    q_off, r_off = _off(q_sizes), _off(r_sizes)
    for exclude in (False, True):
        want, written = KR.rowsum_segmented(q, q_off, r, r_off, GAMMA_EXACT, COEF0, exclude)
        got = run(ctx, q, q_off, r, r_off, GAMMA_EXACT, COEF0, exclude)
        assert written[:nq].all() and not written[nq:].any()
        assert np.array_equal(got[:nq], want[:nq]), np.flatnonzero(got[:nq] != want[:nq])[:10]
        assert _unwritten(got[nq:]).all()
    got = run(ctx, q, q_off, r, r_off, GAMMA_EXACT, COEF0)
    for s, (a, b) in enumerate(zip(q_sizes, r_sizes)):
        if a > 0 and b == 0:
            assert (got[q_off[s]:q_off[s + 1]] == 0.0).all(), s     # an empty reference segment gives 0.0
    # the same rows against themselves, per segment, without the diagonal
    want, _ = KR.rowsum_segmented(r, r_off, r, r_off, GAMMA_EXACT, COEF0, True)
    got = run(ctx, r, r_off, r, r_off, GAMMA_EXACT, COEF0, exclude=True)
    assert np.array_equal(got[:nr], want[:nr]) and _unwritten(got[nr:]).all()
    for s, b in enumerate(r_sizes):
        if b == 1:
            assert got[r_off[s]] == 0.0, s


# offsets the kernel must survive: negative, past n, decreasing.  Read as the header says (clamped to [0, n]; a decreasing pair is
# empty) these segments do not overlap, so every written row has one writer
BAD_Q = [-7, 40, 90, 60, 50]             # n = 130: [0,40) [40,90) [] []       rows 90.. are in no segment
BAD_R = [0, 64, 1000, 2000, 2 ** 31 - 1]  # n = 100: [0,64) [64,100) [] []


def test_offsets_that_decrease_or_exceed_n_touch_nothing_outside_the_tensors(ctx):
    d = 64
    q, r = _ints(11, 130, d), _ints(12, 100, d)
    q_off, r_off = np.array(BAD_Q, np.int32), np.array(BAD_R, np.int32)
    for a, a_off, b, b_off, n_written in ((q, q_off, r, r_off, 90), (r, r_off, q, q_off, 100)):
        want, written = KR.rowsum_segmented(a, a_off, b, b_off, GAMMA_EXACT, COEF0)
        got = run(ctx, a, a_off, b, b_off, GAMMA_EXACT, COEF0)          # (checks the margins)
        assert written[:n_written].all() and not written[n_written:].any()
        assert np.array_equal(got[written], want[written]) and _unwritten(got[~written]).all()


# ------------------------------------------------------------------------------------------------------------- real-valued
REAL_SHAPES = [(130, 64), (130, 3), (130, 256), (257, 67)]


@pytest.mark.parametrize("shift", [0.0, 100.0])
@pytest.mark.parametrize("n,d", REAL_SHAPES)
def test_real_valued_features_stay_within_the_derived_bound(ctx, n, d, shift):
    rs = np.random.RandomState(1000 * d + n)
    q, r = (np.abs(rs.randn(n, d)) + shift).astype(np.float32), (np.abs(rs.randn(n, d)) + shift).astype(np.float32)
    gamma = KR.gamma_of(d)
    off = _off([n])
    eye = np.eye(n, dtype=bool)
    for a, b, exclude in ((q, r, False), (q, q, True)):
        bound, smallest = KR.row_bound(a, b, gamma, COEF0, eye if exclude else None)
        assert (bound < smallest).all(), (bound / smallest).max()        # one dropped or doubled pair cannot hide in the bound
        want, _ = KR.rowsum_segmented(a, off, b, off, gamma, COEF0, exclude)
        got = run(ctx, a, off, b, off, gamma, COEF0, exclude)
        ratio = float((np.abs(got - want) / bound).max())
        print("n %d d %d shift %g exclude %d: bound / smallest term <= %.2e, worst error / bound %.4f"
              % (n, d, shift, exclude, (bound / smallest).max(), ratio))
        assert (np.abs(got - want) <= bound).all(), ratio


# ------------------------------------------------------------------------------------------------------------- other cases
def test_two_eager_calls_and_a_captured_replay_give_the_same_bits(ctx):
    n, m, d = 257, 130, 64
    rng = np.random.default_rng(7)
    x, y = np.abs(rng.standard_normal((n, d))).astype(np.float32), np.abs(rng.standard_normal((m, d))).astype(np.float32)
    sizes_x, sizes_y = [100, 0, 157], [64, 1, 65]
    xd, yd = _dev(ctx, x, np.float32), _dev(ctx, y, np.float32)
    xo, yo = _dev(ctx, _off(sizes_x), np.int32), _dev(ctx, _off(sizes_y), np.int32)
    outs = [(Out(ctx, n), Out(ctx, m)) for _ in range(3)]
    gamma = KR.gamma_of(d)
    torch.cuda.synchronize()

    def call(self_x, cross_y):
        ctx.check(ctx.lib.rcgan_poly3_rowsum(ctx.h, n, n, d, 3, _p(xd), _p(xo), _p(xd), _p(xo), gamma, COEF0, 1, self_x.ptr))
        ctx.check(ctx.lib.rcgan_poly3_rowsum(ctx.h, m, n, d, 3, _p(yd), _p(yo), _p(xd), _p(xo), gamma, COEF0, 0, cross_y.ptr))
    call(*outs[0])
    call(*outs[1])
    ctx.sync()
    ctx.graph_begin()
    try:
        call(*outs[2])
    except BaseException:
        ctx.graph_abort()
        raise
    gid = ctx.graph_end()
    try:
        ctx.sync()
        assert _unwritten(outs[2][0].get()).all() and _unwritten(outs[2][1].get()).all()           # capturing ran nothing
        ctx.graph_launch(gid)
        ctx.sync()
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))
    torch.cuda.synchronize()
    for a, b, c in zip(*outs):
        assert torch.equal(a.raw, b.raw) and torch.equal(a.raw, c.raw)
    want, _ = KR.rowsum_segmented(y, _off(sizes_y), x, _off(sizes_x), gamma, COEF0)
    assert np.allclose(outs[2][1].get(), want, rtol=1e-4, atol=0.0)


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(ctx):
    from rcgan_amd import _lib as L
    x = torch.zeros(8, 4, device=ctx.device)
    off = torch.tensor([0, 8], dtype=torch.int32, device=ctx.device)
    out = Out(ctx, 8)
    torch.cuda.synchronize()
    f = ctx.lib.rcgan_poly3_rowsum
    ok = [8, 8, 4, 1, _p(x), _p(off), _p(x), _p(off), 0.25, 1.0, 0, out.ptr]
    for i, v in ((0, 0), (1, 0), (0, -1), (2, 0), (2, 257), (3, 0), (3, 1025), (4, None), (5, None), (6, None), (7, None), (11, None),
                 (8, float("nan")), (8, float("inf")), (9, float("nan")), (9, -float("inf"))):
        args = list(ok)
        args[i] = v
        assert f(ctx.h, *args) == L.EINVALID_ARG, (i, v)
        assert b"rcgan_poly3_rowsum" in ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    assert _unwritten(out.get()).all()
