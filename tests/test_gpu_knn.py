"""rcgan_knn_radius and rcgan_ball_query (csrc/knn.hip) against brute-force float64 numpy (tests/manifold_ref.py) on the same fp32 inputs.

Exact cases: integer features in [-8, 8], so every squared distance is an integer <= 256 d <= 65 536, exact in fp32 in any order --
radii, counts and nearest distances must EQUAL the reference, ties at the k-th place and on a ball's surface included.

Real-valued cases: the bound is derived, not tuned.  A squared distance is the fp32 sum of (a_i - b_i)^2: one rounding per difference,
one per square, at most d - 1 per sum, so |computed - exact| <= EPS exact with EPS = (d + 3) 2^-24.  Order statistics and minima are
monotone, so radii and nearest distances carry the same bound.  A count is an interval: a pair whose float64 distance lies within
EPS relative of the radius it is compared with is undecided, and decided_in <= count <= decided_in + undecided for every row -- after
asserting that the undecided pairs are at most 0.1 % of all pairs, so that the interval cannot hide a wrong kernel.  The same sets
shifted by +100 in every coordinate must meet the same relative bound (the expanded form |a|^2 + |b|^2 - 2 a.b does not).

Every output sits between two sentinel margins that must come back untouched, and starts out filled with the sentinel: a row the
kernel did not write is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import manifold_ref as MR
from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

MARGIN, SENTINEL = 256, 0xA5
UNWRITTEN_F32 = np.frombuffer(bytes([SENTINEL] * 4), np.float32)[0]       # (-2.87e-16: no distance, radius or -1)
UNWRITTEN_I32 = np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]         # (negative: no count)


def eps_of(d):
    return (d + 3) * 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 26)
    yield c
    c.close()


class Out:
    """n 4-byte outputs between two sentinel margins, themselves filled with the sentinel."""

    def __init__(self, ctx, n, dtype):
        self.n, self.dtype = n, dtype
        self.raw = torch.full((MARGIN + 4 * n + MARGIN,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        self.ptr = C.c_void_p(self.raw.data_ptr() + MARGIN)

    def get(self):
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:MARGIN] == SENTINEL).all() and (raw[MARGIN + 4 * self.n:] == SENTINEL).all(), "a sentinel margin was overwritten"
        return raw[MARGIN:MARGIN + 4 * self.n].view(self.dtype).copy()


def _dev(ctx, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(ctx.device)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run_radius(ctx, x, off, k):
    xd, od = _dev(ctx, x, np.float32), _dev(ctx, off, np.int32)
    out = Out(ctx, len(x), np.float32)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcgan_knn_radius(ctx.h, x.shape[0], x.shape[1], k, len(off) - 1, _p(xd), _p(od), out.ptr))
    ctx.sync()
    return out.get()


def run_ball(ctx, q, q_off, r, r_off, rad, count=True, nearest=True):
    qd, rd = _dev(ctx, q, np.float32), _dev(ctx, r, np.float32)
    qo, ro = _dev(ctx, q_off, np.int32), _dev(ctx, r_off, np.int32)
    radd = _dev(ctx, rad, np.float32) if rad is not None else None
    cnt, near = Out(ctx, len(q), np.int32), Out(ctx, len(q), np.float32)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcgan_ball_query(ctx.h, q.shape[0], r.shape[0], q.shape[1], len(q_off) - 1, _p(qd), _p(qo), _p(rd), _p(ro), _p(radd),
                                       cnt.ptr if count else None, near.ptr if nearest else None))
    ctx.sync()
    return cnt.get(), near.get()


def _ints(seed, n, d, duplicates=False):
    x = np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(np.float32)
    if duplicates and n >= 20:
        x[10:20] = x[0]                   # eleven copies of one row: zero radii up to k = 10
    return x


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------- exact: radii
# one segment: every n of {1, 2, 63, 64, 65, 130, 257}, every d of {1, 3, 64, 67, 256}, every k of {1, 5, 16}
RADIUS_ONE = [(1, 1, 1), (2, 3, 1), (63, 64, 5), (64, 67, 16), (65, 256, 1), (130, 64, 5), (257, 3, 16), (257, 64, 5), (130, 256, 16), (65, 67, 5),
              (64, 1, 5)]
# segment sizes with: an empty segment, a one-row segment, one of exactly k rows, one of k + 1 rows, one across a 64-row boundary
RADIUS_SEGMENTED = [(64, 5, [0, 1, 5, 6, 70, 0, 130, 45]), (3, 1, [1, 2, 0, 90, 37]), (67, 16, [16, 17, 1, 0, 100, 123]),
                    (256, 5, [5, 6, 60, 0, 1, 58])]


@pytest.mark.parametrize("n,d,k", RADIUS_ONE)
def test_radii_of_integer_features_equal_the_reference(ctx, n, d, k):
    x = _ints(n + d + k, n, d, duplicates=True)
    off = _off([n])
    want, written = MR.radii_segmented(x, off, k)
    got = run_radius(ctx, x, off, k)
    assert written.all() and np.array_equal(got.astype(np.float64), want), np.flatnonzero(got != want)[:10]
    if n <= k:
        assert (got == -1.0).all()
    if n >= 20 and k <= 10:
        assert (got[10:20] == 0.0).all() and got[0] == 0.0


@pytest.mark.parametrize("d,k,sizes", RADIUS_SEGMENTED)
def test_radii_per_segment_equal_the_reference(ctx, d, k, sizes):
    n = sum(sizes)
    x = _ints(n + d + k, n, d, duplicates=True)
    off = _off(sizes)
    want, written = MR.radii_segmented(x, off, k)
    got = run_radius(ctx, x, off, k)
    assert written.all() and np.array_equal(got.astype(np.float64), want), np.flatnonzero(got != want)[:10]
    for s, size in enumerate(sizes):
        if 0 < size <= k:
            assert (got[off[s]:off[s + 1]] == -1.0).all(), s


# ------------------------------------------------------------------------------------------------------- exact: ball queries
BALL_ONE = [(1, 2, 64, 1), (2, 1, 3, 1), (63, 64, 256, 16), (64, 65, 67, 5), (65, 63, 1, 1), (130, 257, 64, 5), (257, 130, 3, 16)]
# (d, k, query sizes, reference sizes): segment 0 of the first has queries and no reference; the reference layouts are the radius test's
BALL_SEGMENTED = [(64, 5, [3, 0, 10, 64, 1, 7, 40, 5], [0, 1, 5, 6, 70, 0, 130, 45]),
                  (3, 1, [100, 1, 65, 27, 64], [1, 2, 0, 90, 37]),
                  (67, 16, [60, 70, 0, 2, 125], [16, 17, 1, 0, 96]),
                  (256, 5, [0, 65, 1, 9, 2, 180], [5, 6, 60, 0, 1, 58])]


def _exact_ball(ctx, q, q_off, r, r_off, k):
    rad, _ = MR.radii_segmented(r, r_off, k)                     # (integers or -1: exact as fp32)
    want_c, want_n, written = MR.ball_segmented(q, q_off, r, r_off, rad)
    got_c, got_n = run_ball(ctx, q, q_off, r, r_off, rad)
    assert written.all()
    assert np.array_equal(got_c.astype(np.int64), want_c), np.flatnonzero(got_c != want_c)[:10]
    assert np.array_equal(got_n.astype(np.float64), want_n), np.flatnonzero(got_n != want_n)[:10]
    return got_c, got_n, rad


@pytest.mark.parametrize("nq,nr,d,k", BALL_ONE)
def test_counts_and_nearest_of_integer_features_equal_the_reference(ctx, nq, nr, d, k):
    q, r = _ints(nq + d, nq, d), _ints(nr + d + 1000, nr, d, duplicates=True)
    got_c, _, rad = _exact_ball(ctx, q, _off([nq]), r, _off([nr]), k)
    if nr <= k:
        assert (rad == -1.0).all() and (got_c == 0).all()          # a negative radius never matches
    if d <= 3 and nr > k:
        # ties on a ball's surface do occur here: this case cannot pass by luck
        D = MR.dist2(q, r)
        assert (D == rad[None, :]).any()


@pytest.mark.parametrize("d,k,q_sizes,r_sizes", BALL_SEGMENTED)
def test_counts_and_nearest_per_segment_equal_the_reference(ctx, d, k, q_sizes, r_sizes):
    nq, nr = sum(q_sizes), sum(r_sizes)
    assert nq != nr
    q, r = _ints(nq + d, nq, d), _ints(nr + d + 1000, nr, d, duplicates=True)
    q_off, r_off = _off(q_sizes), _off(r_sizes)
    got_c, got_n, _ = _exact_ball(ctx, q, q_off, r, r_off, k)
    for s, (a, b) in enumerate(zip(q_sizes, r_sizes)):
        if a > 0 and b == 0:
            assert (got_c[q_off[s]:q_off[s + 1]] == 0).all() and np.isposinf(got_n[q_off[s]:q_off[s + 1]]).all(), s
        if a > 0 and 0 < b <= k:
            assert (got_c[q_off[s]:q_off[s + 1]] == 0).all() and np.isfinite(got_n[q_off[s]:q_off[s + 1]]).all(), s


def test_either_output_may_be_left_out(ctx):
    q, r = _ints(1, 65, 64), _ints(2, 130, 64)
    q_off, r_off = _off([65]), _off([130])
    rad, _ = MR.radii_segmented(r, r_off, 5)
    both = run_ball(ctx, q, q_off, r, r_off, rad)
    only_c, untouched_n = run_ball(ctx, q, q_off, r, r_off, rad, nearest=False)
    untouched_c, only_n = run_ball(ctx, q, q_off, r, r_off, None, count=False)          # (no count: no radii needed)
    assert np.array_equal(only_c, both[0]) and np.array_equal(only_n, both[1])
    assert (untouched_n.view(np.int32) == UNWRITTEN_I32).all() and (untouched_c == UNWRITTEN_I32).all()


# ----------------------------------------------------------------------------------------------------------- real-valued
REAL_SHAPES = [(130, 197, 64, 5), (65, 63, 3, 1), (257, 300, 67, 3)]


@pytest.mark.parametrize("shift", [0.0, 100.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("nq,nr,d,k", REAL_SHAPES)
def test_real_valued_features_stay_within_the_derived_bound(ctx, nq, nr, d, k, seed, shift):
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((nr, d)) + shift).astype(np.float32)
    q = (1.1 * rng.standard_normal((nq, d)) + 0.2 + shift).astype(np.float32)
    eps = eps_of(d)
    q_off, r_off = _off([nq]), _off([nr])
    # radii of the reference set and of the query set
    for x, off in ((r, r_off), (q, q_off)):
        want, _ = MR.radii_segmented(x, off, k)
        got = run_radius(ctx, x, off, k).astype(np.float64)
        assert (np.abs(got - want) <= eps * want).all(), (np.abs(got - want) / want).max() / eps
    # counts and nearest distances, the radii an input array
    rad = MR.radii_segmented(r, r_off, k)[0].astype(np.float32)
    inside, open_ = MR.undecided(q, q_off, r, r_off, rad, eps)
    assert open_.sum() <= 1e-3 * nq * nr, open_.sum()                        # a condition on the test's data, asserted on the host
    _, want_n, _ = MR.ball_segmented(q, q_off, r, r_off, rad)
    got_c, got_n = run_ball(ctx, q, q_off, r, r_off, rad)
    print("undecided pairs %d of %d; worst nearest error / bound %.3f" % (open_.sum(), nq * nr, (np.abs(got_n - want_n) / (eps * want_n)).max()))
    assert (np.abs(got_n.astype(np.float64) - want_n) <= eps * want_n).all()
    assert ((inside <= got_c) & (got_c <= inside + open_)).all(), np.flatnonzero((got_c < inside) | (got_c > inside + open_))[:10]


# ----------------------------------------------------------------------------------------------------------- other cases
def test_two_eager_calls_and_a_captured_replay_give_the_same_bits(ctx):
    n, m, d, k = 257, 130, 64, 5
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    sizes_x, sizes_y = [100, 0, 157], [64, 1, 65]
    xd, yd = _dev(ctx, x, np.float32), _dev(ctx, y, np.float32)
    xo, yo = _dev(ctx, _off(sizes_x), np.int32), _dev(ctx, _off(sizes_y), np.int32)
    outs = [(Out(ctx, n, np.float32), Out(ctx, m, np.int32), Out(ctx, m, np.float32)) for _ in range(3)]
    torch.cuda.synchronize()

    def call(rad, cnt, near):
        ctx.check(ctx.lib.rcgan_knn_radius(ctx.h, n, d, k, 3, _p(xd), _p(xo), rad.ptr))
        ctx.check(ctx.lib.rcgan_ball_query(ctx.h, m, n, d, 3, _p(yd), _p(yo), _p(xd), _p(xo), rad.ptr, cnt.ptr, near.ptr))
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
        assert (outs[2][0].get().view(np.int32) == UNWRITTEN_I32).all()           # capturing ran nothing
        ctx.graph_launch(gid)
        ctx.sync()
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))
    torch.cuda.synchronize()
    for a, b, c in zip(*outs):
        assert torch.equal(a.raw, b.raw) and torch.equal(a.raw, c.raw)
    want, _ = MR.radii_segmented(x, _off(sizes_x), k)
    assert (np.abs(outs[2][0].get() - want) <= eps_of(d) * want).all()


# offsets the kernel must survive: negative, past n, decreasing.  Read as the header says (clamped to [0, n]; a decreasing pair is
# empty) these segments do not overlap, so every written row has one writer
BAD_Q = [-7, 40, 90, 60, 50]             # n = 130: [0,40) [40,90) [] []       rows 90.. are in no segment
BAD_R = [0, 64, 1000, 2000, 2 ** 31 - 1]  # n = 100: [0,64) [64,100) [] []


def test_offsets_that_decrease_or_exceed_n_touch_nothing_outside_the_tensors(ctx):
    d, k = 64, 5
    q, r = _ints(11, 130, d), _ints(12, 100, d)
    q_off, r_off = np.array(BAD_Q, np.int32), np.array(BAD_R, np.int32)
    for x, off in ((q, q_off), (r, r_off)):
        want, written = MR.radii_segmented(x, off, k)
        got = run_radius(ctx, x, off, k)                    # (checks the margins)
        assert np.array_equal(got[written].astype(np.float64), want[written])
        assert (got[~written].view(np.int32) == UNWRITTEN_I32).all()
    rad = MR.radii_segmented(r, r_off, k)[0]
    want_c, want_n, written = MR.ball_segmented(q, q_off, r, r_off, rad)
    got_c, got_n = run_ball(ctx, q, q_off, r, r_off, rad)
    assert written[:90].all() and not written[90:].any()
    assert np.array_equal(got_c[written].astype(np.int64), want_c[written]) and np.array_equal(got_n[written].astype(np.float64), want_n[written])
    assert (got_c[~written] == UNWRITTEN_I32).all() and (got_n[~written].view(np.int32) == UNWRITTEN_I32).all()


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(ctx):
    from rcgan_amd import _lib as L
    x = torch.zeros(8, 4, device=ctx.device)
    off = torch.tensor([0, 8], dtype=torch.int32, device=ctx.device)
    rad, cnt, near = Out(ctx, 8, np.float32), Out(ctx, 8, np.int32), Out(ctx, 8, np.float32)
    torch.cuda.synchronize()
    f = ctx.lib.rcgan_knn_radius
    for args in ((0, 4, 1, 1, _p(x), _p(off), rad.ptr), (8, 0, 1, 1, _p(x), _p(off), rad.ptr), (8, 257, 1, 1, _p(x), _p(off), rad.ptr),
                 (8, 4, 0, 1, _p(x), _p(off), rad.ptr), (8, 4, 17, 1, _p(x), _p(off), rad.ptr), (8, 4, 1, 0, _p(x), _p(off), rad.ptr),
                 (8, 4, 1, 1025, _p(x), _p(off), rad.ptr), (8, 4, 1, 1, None, _p(off), rad.ptr), (8, 4, 1, 1, _p(x), None, rad.ptr),
                 (8, 4, 1, 1, _p(x), _p(off), None)):
        assert f(ctx.h, *args) == L.EINVALID_ARG, args
        assert b"rcgan_knn_radius" in ctx.lib.rcgan_last_error(ctx.h)
    g = ctx.lib.rcgan_ball_query
    ok = [8, 8, 4, 1, _p(x), _p(off), _p(x), _p(off), rad.ptr, cnt.ptr, near.ptr]
    for i, v in ((0, 0), (1, 0), (2, 0), (2, 257), (3, 0), (3, 1025), (4, None), (5, None), (6, None), (7, None), (8, None)):
        args = list(ok)
        args[i] = v
        assert g(ctx.h, *args) == L.EINVALID_ARG, (i, v)
        assert b"rcgan_ball_query" in ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    for o in (rad, cnt, near):
        assert (o.get().view(np.int32) == UNWRITTEN_I32).all()
