"""rcgan_nn_u8 (csrc/nn_u8.hip) against the brute-force int64 restatement (tests/neighbours_ref.py) on the same uint8 rows.

The kernel's result is exact, so every comparison is equality of the 64-bit keys (dist2 << 32 | index): no tolerance anywhere.
Covered: feature sizes below one k-step, with a k tail, MNIST's and CIFAR's; zero distances and the lowest-index tie rule; the
extremes of the int32 arithmetic; several reference tiles and splits with the nearest row planted around every multiple of 64;
segments (empty, single-row, decreasing, beyond n, rows outside every segment); exclusion of the own row; an asymmetric plant that a
swap of the operands or of row and column cannot pass; eager against replayed bits.

Every buffer lies between tests/guard.py margins.  ``best`` starts out as the guard's fill, which is also the kernel's "no candidate"
value, so the segment test writes another pattern into it first: rows outside every segment must keep it, rows inside must not."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import neighbours_ref as NR
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

PATTERN = np.uint64(0x0123456789ABCDEF)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 20)                 # (its own arena is replaced by the guarded one)
    cm = guarded(c, arena_bytes=64 << 20, ws_bytes=1 << 20)
    c.guard = cm.__enter__()
    yield c
    cm.__exit__(None, None, None)
    c.close()


def _bytes(ctx, a):
    from rcgan_amd.runtime import DT
    a = np.ascontiguousarray(a, np.uint8)
    t = DT(ctx.arena.alloc(a.size), a.shape, "u8", ctx.arena.buf)
    off = t.ptr - t.base.data_ptr()
    with torch.cuda.stream(ctx.stream):
        t.base.view(torch.uint8).reshape(-1)[off:off + a.size].copy_(torch.from_numpy(a.reshape(-1)))
    return t


def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _fresh(ctx):
    ctx.guard.clear()
    ctx.new_step()


def _keys(ctx, out):
    return np.ascontiguousarray(ctx.download(out).astype(np.int32)).view(np.uint64).reshape(-1)


def launch(ctx, q, r, q_off, r_off, exclude, out, nq=None, nr=None):
    nq, nr = q.shape[0] if nq is None else nq, r.shape[0] if nr is None else nr
    ctx.check(ctx.lib.rcgan_nn_u8(ctx.h, nq, nr, q.shape[1], q_off.shape[0] - 1, _p(q), _p(q_off), _p(r), _p(r_off), int(exclude), _p(out)))


def run(ctx, q, r, q_off=None, r_off=None, exclude=False, prefill=None, same=False):
    """-> the uint64 keys after one call.  same: q and r are ONE device buffer (exclusion's case)."""
    _fresh(ctx)
    q_off = [0, len(q)] if q_off is None else q_off
    r_off = [0, len(r)] if r_off is None else r_off
    dq = _bytes(ctx, q)
    dr = dq if same else _bytes(ctx, r)
    dqo, dro = ctx.upload(np.asarray(q_off, np.int64)), ctx.upload(np.asarray(r_off, np.int64))
    out = ctx.empty((len(q), 2), "i32")                 # starts out as the guard's fill: all-ones
    if prefill is not None:
        with torch.cuda.stream(ctx.stream):
            ctx.view(out).copy_(torch.from_numpy(np.full(len(q), prefill, np.uint64).view(np.int32).reshape(-1, 2)))
    launch(ctx, dq, dr, dqo, dro, exclude, out)
    ctx.sync()
    ctx.guard.check()
    return _keys(ctx, out)


def same_keys(got, want):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d of %d keys differ, first at row %d: got dist2 %d index %d, expected dist2 %d index %d" % (
        len(bad), len(got), bad[0], got[bad[0]] >> np.uint64(32), got[bad[0]] & np.uint64(0xFFFFFFFF),
        want[bad[0]] >> np.uint64(32), want[bad[0]] & np.uint64(0xFFFFFFFF))


# ------------------------------------------------------------------------------------------------------- feature sizes
@pytest.mark.parametrize("d", [16, 48, 784, 3072])
def test_random_rows_planted_copies_and_the_lowest_index_among_duplicates(ctx, d):
    rs = np.random.RandomState(d)
    nq, nr = 150, 300
    q, r = rs.randint(0, 256, size=(nq, d), dtype=np.uint8), rs.randint(0, 256, size=(nr, d), dtype=np.uint8)
    got = run(ctx, q, r)
    same_keys(got, NR.best(q, r))
    # a few rows of r copied into q: distance 0
    q2 = q.copy()
    src = np.array([0, 31, 32, 127, 128, 255, 256, 299])
    dst = np.array([149, 3, 64, 65, 127, 128, 0, 77])
    q2[dst] = r[src]
    got = run(ctx, q2, r)
    same_keys(got, NR.best(q2, r))
    assert (got[dst] == src.astype(np.uint64)).all()                 # dist2 0 in the upper half, the copied row in the lower
    # one row of r present at a lower and at a higher index: the lower one is reported
    r3, q3 = r.copy(), q.copy()
    r3[40] = r3[260] = r3[131] = q3[5]
    r3[290] = r3[129] = q3[140]
    got = run(ctx, q3, r3)
    same_keys(got, NR.best(q3, r3))
    assert got[5] == np.uint64(40) and got[140] == np.uint64(129)


# ------------------------------------------------------------------------------------------------------------ extremes
def test_the_largest_distances_and_rows_of_centred_zero(ctx):
    for d, n, want in ((3072, 3, 199756800), (12288, 2, 799027200)):
        q, r = np.zeros((n, d), np.uint8), np.full((n, d), 255, np.uint8)
        for a, b in ((q, r), (r, q)):
            got = run(ctx, a, b)
            assert (got == np.uint64(want << 32)).all(), (d, got)      # index 0: every reference row is equally far
            same_keys(got, NR.best(a, b))
    # mixed extremes at full length: the inner product at both ends of its range, the norms at their largest
    d = 12288
    rows = np.stack([np.zeros(d), np.full(d, 255), np.full(d, 128), np.arange(d) % 2 * 255, np.full(d, 127)]).astype(np.uint8)
    same_keys(run(ctx, rows, rows[::-1].copy()), NR.best(rows, rows[::-1].copy()))
    same_keys(run(ctx, rows, rows, exclude=True, same=True), NR.best(rows, rows, exclude=True))
    # all-128 rows have centred value zero, as the padding of a tile has: a padding row must never be reported
    d = 48
    rs = np.random.RandomState(5)
    q = np.full((7, d), 128, np.uint8)
    r = rs.randint(0, 256, size=(5, d), dtype=np.uint8)                 # 123 padding rows behind them
    got = run(ctx, q, r)
    same_keys(got, NR.best(q, r))
    assert (got >> np.uint64(32)).min() > 0 and (got & np.uint64(0xFFFFFFFF)).max() < 5
    r[3] = 128
    got = run(ctx, q, r)
    assert (got == np.uint64(3)).all()
    r130 = np.concatenate([rs.randint(0, 256, size=(129, d), dtype=np.uint8), np.full((1, d), 128, np.uint8)])    # the last row of a short second tile
    assert (run(ctx, q, r130) == np.uint64(129)).all()


# ------------------------------------------------------------------------------------- several reference tiles and splits
def test_the_nearest_row_planted_around_every_multiple_of_64_of_a_long_reference_segment(ctx):
    rs = np.random.RandomState(11)
    nq, nr, d = 130, 1100, 48
    q, r = rs.randint(0, 256, size=(nq, d), dtype=np.uint8), rs.randint(0, 256, size=(nr, d), dtype=np.uint8)
    places = sorted({0, 127, 128, 1099} | {p for k in range(1, 18) for p in (64 * k - 1, 64 * k, 64 * k + 1) if p < nr})
    assert len(places) <= nq
    queries = rs.permutation(nq)[:len(places)]
    for i, p in zip(queries, places):
        r[p] = q[i]
        r[p, p % d] ^= 1                                              # distance 1: no random row comes close
    got = run(ctx, q, r)
    same_keys(got, NR.best(q, r))
    assert (got[queries] == ((np.uint64(1) << np.uint64(32)) | np.array(places, np.uint64))).all()
    # exact duplicates in different tiles and splits: the lowest index
    r2 = r.copy()
    r2[1090] = r2[700] = r2[129] = q[int(queries[0])]
    got = run(ctx, q, r2)
    same_keys(got, NR.best(q, r2))
    assert got[int(queries[0])] == np.uint64(129)


# ------------------------------------------------------------------------------------------------------------ segments
def test_segments_empty_single_decreasing_beyond_n_and_rows_outside_every_segment(ctx):
    rs = np.random.RandomState(12)
    nq, nr, d = 200, 500, 32
    q, r = rs.randint(0, 256, size=(nq, d), dtype=np.uint8), rs.randint(0, 256, size=(nr, d), dtype=np.uint8)
    # queries: rows 0..9 in no segment; 10..70; one row; 71..130 (its references are empty); 130..n (offset beyond n); a decreasing pair
    q_off = [10, 70, 71, 130, 100000, 180]
    r_off = [-5, 200, 330, 330, 500, 400]
    for exclude in (False, True):
        got = run(ctx, q, r, q_off, r_off, exclude=exclude, prefill=PATTERN)
        want = NR.best(q, r, q_off, r_off, exclude=exclude, fill=PATTERN)
        same_keys(got, want)
        assert (got[:10] == PATTERN).all() and (got[71:130] == NR.ALL_ONES).all() and (got[10:71] != NR.ALL_ONES).all()
        idx = (got & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (idx[10:70] < 200).all() and 200 <= idx[70] < 330 and (idx[130:] >= 330).all() and (idx[130:] < 500).all()
    # every query segment empty or decreasing: nothing is written
    got = run(ctx, q, r, [50, 50, 20], [0, 100, 500], prefill=PATTERN)
    assert (got == PATTERN).all()
    # three unequal segments spanning several query tiles, well formed: every row written
    q_off, r_off = [0, 3, 140, 200], [0, 260, 261, 500]
    got = run(ctx, q, r, q_off, r_off, prefill=PATTERN)
    same_keys(got, NR.best(q, r, q_off, r_off))
    assert (got != PATTERN).all() and (got[3:140] & np.uint64(0xFFFFFFFF) == np.uint64(260)).all()


# ----------------------------------------------------------------------------------------------------------- exclusion
def test_exclusion_leaves_out_the_own_row_and_only_that(ctx):
    rs = np.random.RandomState(13)
    n, d = 300, 48
    x = rs.randint(0, 256, size=(n, d), dtype=np.uint8)
    x[200] = x[150]                                                      # an exact duplicate: each reports the other at distance 0
    x[290] = x[5]                                                        # ... also across two tiles
    off = [0, 1, 140, 300]                                               # a one-row segment: no candidate
    got = run(ctx, x, x, off, off, exclude=True, same=True)
    same_keys(got, NR.best(x, x, off, off, exclude=True))
    idx = (got & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert got[0] == NR.ALL_ONES and (idx[1:] != np.arange(1, n)).all()
    assert got[150] == np.uint64(200) and got[200] == np.uint64(150)
    assert got[5] != np.uint64(290) and got[290] != np.uint64(5)         # (rows 5 and 290 lie in different segments)
    got = run(ctx, x, x, exclude=True, same=True)
    same_keys(got, NR.best(x, x, exclude=True))
    assert got[5] == np.uint64(290) and got[290] == np.uint64(5)
    # without exclusion every row reports itself -- or an earlier duplicate of itself
    got = run(ctx, x, x, same=True)
    want = np.arange(n, dtype=np.uint64)
    want[200], want[290] = 150, 5
    assert (got == want).all()


# --------------------------------------------------------------------------------------------------------- orientation
def test_an_asymmetric_plant_pins_which_operand_is_the_row_and_which_the_column(ctx):
    rs = np.random.RandomState(14)
    nq, nr, d = 100, 170, 64
    r = rs.randint(0, 256, size=(nr, d), dtype=np.uint8)
    target = (7 * np.arange(nq) + 3) % nr
    q = r[target].copy()
    q[np.arange(nq), np.arange(nq) % d] ^= 1
    got = run(ctx, q, r)
    same_keys(got, NR.best(q, r))
    assert (got == ((np.uint64(1) << np.uint64(32)) | target.astype(np.uint64))).all()


# -------------------------------------------------------------------------------------------------------------- replay
def test_two_eager_runs_and_a_graph_replay_give_the_same_bits(ctx):
    rs = np.random.RandomState(15)
    nq, nr, d = 130, 1100, 784
    q, r = rs.randint(0, 4, size=(nq, d), dtype=np.uint8), rs.randint(0, 4, size=(nr, d), dtype=np.uint8)     # few levels: many ties
    _fresh(ctx)
    dq, dr = _bytes(ctx, q), _bytes(ctx, r)
    dqo, dro = ctx.upload(np.array([0, 60, nq])), ctx.upload(np.array([0, 500, nr]))
    outs = [ctx.empty((nq, 2), "i32") for _ in range(3)]
    launch(ctx, dq, dr, dqo, dro, False, outs[0])
    launch(ctx, dq, dr, dqo, dro, False, outs[1])
    ctx.sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=ctx.stream):
        launch(ctx, dq, dr, dqo, dro, False, outs[2])
    ctx.sync()
    graph.replay()
    torch.cuda.synchronize()
    ctx.guard.check()
    a, b, c = (_keys(ctx, o) for o in outs)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    same_keys(c, NR.best(q, r, [0, 60, nq], [0, 500, nr]))
    del graph


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(ctx):
    from rcgan_amd import _lib as L
    _fresh(ctx)
    q, r = _bytes(ctx, np.zeros((8, 32), np.uint8)), _bytes(ctx, np.zeros((8, 32), np.uint8))
    off = ctx.upload(np.array([0, 8]))
    out = ctx.empty((8, 2), "i32")
    with torch.cuda.stream(ctx.stream):
        ctx.view(out).fill_(7)
    ok = [8, 8, 32, 1, _p(q), _p(off), _p(r), _p(off), 0, _p(out)]
    for i, v in ((0, 0), (1, -1), (2, 0), (2, 8), (2, 24), (2, 12304), (3, 0), (3, 1025), (4, None), (5, None), (6, None), (7, None), (9, None),
                 (4, C.c_void_p(q.ptr + 8)), (6, C.c_void_p(r.ptr + 4)), (9, C.c_void_p(out.ptr + 4))):
        args = list(ok)
        args[i] = v
        assert ctx.lib.rcgan_nn_u8(ctx.h, *args) == L.EINVALID_ARG, (i, v)
        assert b"rcgan_nn_u8" in ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    ctx.guard.check()
    assert (ctx.download(out) == 7).all()
