"""rcgan_msssim_pairs (csrc/msssim.hip) against the float64 restatement (tests/msssim_ref.py) on the same uint8 images.

Twelve images per shape: four template images (crops / one channel for the smaller shapes), one of them plus noise, uniform noise,
constants 0, 255 and 7, a 0/255 checkerboard (the largest second moments a window can hold) and its inverse, and a half plane plus
small noise (flat regions far from the image's mean).  About forty pairs: every image with itself, black against white, the
checkerboard against its inverse, repeated pairs, random pairs, and two rows with an index outside [0, n) -- they must come back nan
with their neighbours intact.  Shapes: 32x32x3 (the declared upper bound, 16-byte loads), 28x28x1 (odd at the third level),
16x16x1 (the smallest: windows 11, 8, 4, 2, 1), 17x23x3 (odd at the first level, not square, images that are no multiple of 16 bytes:
the byte loads), and 16x32x3 / 32x17x1 (one side at each bound).

All ten outputs of every pair are held to TOL = 1e-4, the bound derived in the header of csrc/msssim.hip from the kernel's arithmetic
(no difference of second moments; fp32 fused multiply-add chains of at most 11 terms).  The error measured on the MI355X is printed.

Every buffer lies between tests/guard.py margins; the output starts out as the guard's fill (nan): a value the kernel did not write
is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import msssim_ref as MR
from tests.gpu_util import make_ctx
from tests.guard import guarded

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(32, 32, 3), (28, 28, 1), (16, 16, 1), (17, 23, 3), (16, 32, 3), (32, 17, 1)]
N = 12


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 20)                 # (its own arena is replaced by the guarded one)
    cm = guarded(c, arena_bytes=64 << 20, ws_bytes=1 << 20)
    c.guard = cm.__enter__()
    yield c
    cm.__exit__(None, None, None)
    c.close()


def images_of(shape):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as DT
    h, w, c = shape
    rs = np.random.RandomState(1000 * h + 10 * w + c)
    t = DT.template_images(rs, np.array([0, 0, 1, 2])).reshape(4, 3, 32, 32).transpose(0, 2, 3, 1)[:, :h, :w, :c]
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.broadcast_to((((yy + xx) % 2) * 255)[..., None], shape)
    plane = np.broadcast_to(((xx >= w // 2) * 255)[..., None], shape)
    x = list(t) + [np.clip(np.rint(t[0] + 20.0 * rs.randn(*shape)), 0, 255), rs.randint(0, 256, size=shape), np.zeros(shape), np.full(shape, 255),
                   np.full(shape, 7), board, 255 - board, np.clip(plane + rs.randint(-2, 3, size=shape), 0, 255)]
    assert len(x) == N
    return np.ascontiguousarray(np.stack(x), np.uint8)


def pairs_of(shape):
    rs = np.random.RandomState(sum(shape))
    p = [(i, i) for i in range(N)] + [(6, 7), (7, 6), (9, 10), (6, 8), (0, 1), (0, 1), (0, 1), (2, 3), (0, 4), (0, 5), (11, 6), (11, 9)]
    p += [tuple(int(v) for v in rs.randint(0, N, size=2)) for _ in range(14)]
    p[20], p[33] = (3, N), (-1, 2)                       # out of range on either side; rows 19, 21, 32, 34 are ordinary pairs
    return np.array(p, np.int32)


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


def launch(ctx, x, pairs, out, shape, n=N):
    ctx.check(ctx.lib.rcgan_msssim_pairs(ctx.h, n, shape[0], shape[1], shape[2], pairs.shape[0], _p(x), _p(pairs), _p(out)))


def run(ctx, images, pairs):
    from rcgan_amd import _lib as L
    _fresh(ctx)
    x, p = _bytes(ctx, images), ctx.upload(pairs)
    out = ctx.empty((len(pairs), 2, 5), L.F32)           # starts out as nan (the guard's fill)
    launch(ctx, x, p, out, images.shape[1:], len(images))
    ctx.sync()
    ctx.guard.check()
    return ctx.download(out), out


@pytest.fixture(scope="module")
def reference():
    """The restatement's [P, 2, 5] of every shape's pairs, computed once."""
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = (images_of(shape), pairs_of(shape), MR.scales(images_of(shape), pairs_of(shape)))
        return made[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_every_pair_is_within_the_derived_bound(ctx, reference, shape):
    images, pairs, want = reference(shape)
    got, out = run(ctx, images, pairs)
    bad = np.isnan(want[:, 0, 0])
    assert bad.tolist() == [k in (20, 33) for k in range(len(pairs))]
    assert np.isnan(got[bad]).all() and ctx.guard.unwritten(out) == 0            # (the kernel's nan is not the guard's fill pattern: every row was written)
    assert np.isfinite(got[~bad]).all()
    err = np.abs(got[~bad].astype(np.float64) - want[~bad])
    print("%dx%dx%d: %d pairs, largest error of a per-scale mean %.3e (bound %.0e), per scale %s"
          % (shape + (int((~bad).sum()), err.max(), TOL, np.array2string(err.max(axis=(0, 1)), precision=2))))
    assert (err <= TOL).all(), (err.max(), np.unravel_index(err.argmax(), err.shape))
    for k in range(N):                                                            # an image against itself: exactly 1
        assert (got[k] == 1.0).all(), (k, got[k])
    assert np.array_equal(got[16], got[17]) and np.array_equal(got[17], got[18])     # a repeated pair gives the same bits


def test_a_single_pair_and_a_list_of_out_of_range_pairs_only(ctx, reference):
    shape = (28, 28, 1)
    images, _, _ = reference(shape)
    got, out = run(ctx, images, np.array([[4, 11]], np.int32))
    assert ctx.guard.unwritten(out) == 0
    assert np.abs(got[0] - MR.pair_scales(images[4], images[11])).max() <= TOL
    got, out = run(ctx, images, np.array([[N, 0], [0, N], [2 ** 31 - 1, -2 ** 31]], np.int32))
    assert np.isnan(got).all() and ctx.guard.unwritten(out) == 0


def test_two_eager_runs_and_a_torch_graph_replay_give_the_same_bits(ctx, reference):
    from rcgan_amd import _lib as L
    shape = (32, 32, 3)
    images, pairs, want = reference(shape)
    _fresh(ctx)
    x, p = _bytes(ctx, images), ctx.upload(pairs)
    outs = [ctx.empty((len(pairs), 2, 5), L.F32) for _ in range(3)]
    launch(ctx, x, p, outs[0], shape)
    launch(ctx, x, p, outs[1], shape)
    ctx.sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=ctx.stream):
        launch(ctx, x, p, outs[2], shape)
    ctx.sync()
    assert ctx.guard.unwritten(outs[2]) == outs[2].size                           # capturing ran nothing
    graph.replay()
    torch.cuda.synchronize()
    ctx.guard.check()
    a, b, c = (ctx.download(o) for o in outs)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    ok = ~np.isnan(want[:, 0, 0])
    assert np.abs(c[ok] - want[ok]).max() <= TOL
    del graph


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing(ctx, reference):
    from rcgan_amd import _lib as L
    shape = (32, 32, 3)
    images, pairs, _ = reference(shape)
    _fresh(ctx)
    x, p = _bytes(ctx, images), ctx.upload(pairs)
    out = ctx.empty((len(pairs), 2, 5), L.F32)
    ok = [N, 32, 32, 3, len(pairs), _p(x), _p(p), _p(out)]
    for i, v in ((0, 0), (0, -1), (1, 15), (1, 33), (2, 15), (2, 33), (3, 2), (3, 0), (3, 4), (4, 0), (4, -3), (5, None), (6, None), (7, None)):
        args = list(ok)
        args[i] = v
        assert ctx.lib.rcgan_msssim_pairs(ctx.h, *args) == L.EINVALID_ARG, (i, v)
        assert b"rcgan_msssim_pairs" in ctx.lib.rcgan_last_error(ctx.h)
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(out) == out.size
