"""The guard-band checker (tests/guard.py) itself, on host tensors: every kind of violation it exists to catch is written by the test
into the structures it builds on torch.device("cpu"), and check() must fail naming the right allocation and offset -- and pass when only
bodies are written.  No kernel runs and nothing on a GPU is made to misbehave."""
import numpy as np
import pytest
import torch

import rcgan_amd  # noqa: F401
from rcgan_amd import _lib as L
from rcgan_amd.runtime import ALIGN, DT
from tests import guard as G

CPU = torch.device("cpu")


class StubContext:
    """What guarded() touches of a runtime.Context, without a device."""

    def __init__(self):
        self.arena = "the original arena"
        self.ws_ptr, self.ws_bytes = 1234, 5678
        self.stream = None
        self.capturing = False

    def persistent(self, shape, dtype=L.F32, fill=None):
        raise AssertionError("the original persistent() must not be reached under guard")

    def empty(self, shape, dtype):          # Context.empty, restated
        n = int(np.prod(shape)) if shape else 1
        return DT(self.arena.alloc(max(n, 1) * (4 if dtype in (L.F32, "i32") else 2)), shape, dtype, self.arena.buf)


@pytest.fixture()
def gc():
    ctx = StubContext()
    with G.guarded(ctx, device=CPU, arena_bytes=8 << 20, ws_bytes=1 << 20) as g:
        yield g, ctx
    assert ctx.arena == "the original arena" and (ctx.ws_ptr, ctx.ws_bytes) == (1234, 5678)
    assert "persistent" not in ctx.__dict__          # the class's method is visible again


def _bytes(t):
    """The body of a DT as a writable uint8 view."""
    off = t.ptr - t.base.data_ptr()
    return t.base.view(torch.uint8).reshape(-1)[off:off + t.nbytes]


def _poke(t, rel):
    """Write one byte at `rel` bytes from the start of the body of t (negative: in front of it)."""
    off = t.ptr - t.base.data_ptr()
    t.base.view(torch.uint8).reshape(-1)[off + rel] = 0


def test_layout_and_fill(gc):
    g, ctx = gc
    assert isinstance(ctx.arena, G.GuardedArena) and ctx.ws_bytes == 1 << 20 and ctx.ws_ptr % 256 == 0
    assert bool((ctx.arena.buf == 0xFF).all())
    a = ctx.empty((3, 5), L.BF16)
    b = ctx.empty((7,), L.F32)
    assert a.ptr % ALIGN == 0 and b.ptr % ALIGN == 0
    assert a.ptr - ctx.arena.base >= G.MARGIN and b.ptr - (a.ptr + a.nbytes) >= 2 * G.MARGIN
    assert G.MARGIN % ALIGN == 0 and G.MARGIN >= 64 << 10 and G.WS_MARGIN == 1 << 20
    assert ctx.arena.off == ctx.arena.peak >= b.ptr - ctx.arena.base + b.nbytes + G.MARGIN
    # the fill is a NaN in every float format and -1 as int32
    assert torch.isnan(_bytes(b).view(torch.float32)).all() and torch.isnan(_bytes(a).view(torch.bfloat16)).all()
    assert torch.isnan(_bytes(a).view(torch.float16)).all() and bool((_bytes(b).view(torch.int32) == -1).all())
    g.check()


def test_bodies_may_be_written_and_reset_refills(gc):
    g, ctx = gc
    a, b = ctx.empty((100,), L.F32), ctx.empty((33,), L.BF16)
    p = ctx.persistent((4, 4), L.F32, fill=0.0)
    assert p.base is not None and float(_bytes(p).view(torch.float32).abs().sum()) == 0.0        # fill= honoured for the body
    for t in (a, b, p):
        _bytes(t).zero_()
    g.ws.body().zero_()
    g.check()
    with g.workspace(1000) as fr:
        assert ctx.ws_bytes == 1000 and ctx.ws_ptr % 256 == 0 and fr.body().numel() == 1000
        fr.body().zero_()
        g.check()
    assert ctx.ws_bytes == 1 << 20
    peak = ctx.arena.peak
    ctx.arena.reset()
    assert ctx.arena.off == 0 and ctx.arena.peak == peak and bool((ctx.arena.buf[:peak + G.SLACK] == 0xFF).all())
    assert bool((g.ws.body() == 0xFF).all())
    g.check()


def test_one_byte_past_a_body(gc):
    g, ctx = gc
    a, b = ctx.empty((10,), L.F32), ctx.empty((10,), L.F32)
    _poke(a, a.nbytes)
    with pytest.raises(AssertionError, match=r"0 bytes past the end of arena allocation #0 \(offset \d+, 40 bytes\)"):
        g.check()


def test_reset_checks_before_it_refills(gc):
    g, ctx = gc
    a = ctx.empty((10,), L.F32)
    _poke(a, a.nbytes + 3)
    with pytest.raises(AssertionError, match=r"3 bytes past the end of arena allocation #0"):
        ctx.arena.reset()           # (Context.new_step in the middle of a test body)
    g.clear()                       # a fresh start forgets it
    g.check()
    assert ctx.arena.off == 0 and not ctx.arena.bodies


def test_one_byte_before_a_body(gc):
    g, ctx = gc
    a, b = ctx.empty((10,), L.F32), ctx.empty((6,), L.BF16)
    _poke(b, -1)
    with pytest.raises(AssertionError, match=r"1 bytes before the start of arena allocation #1 \(offset \d+, 12 bytes\)"):
        g.check()


def test_write_into_space_never_allocated(gc):
    g, ctx = gc
    a = ctx.empty((10,), L.F32)
    _poke(a, a.nbytes + (200 << 10))
    with pytest.raises(AssertionError, match=r"%d bytes past the end of arena allocation #0 .*never allocated" % (200 << 10)):
        g.check()


def test_write_at_workspace_byte_nbytes(gc):
    g, ctx = gc
    with g.workspace(4096 + 40) as fr:
        fr.raw[fr.lead + ctx.ws_bytes] = 7
        with pytest.raises(AssertionError, match=r"0 bytes past the end of tight workspace \(4136 bytes\) \(workspace byte 4136\); value 0x07"):
            g.check()
        fr.raw[fr.lead + ctx.ws_bytes] = 0xFF
        fr.raw[fr.lead - 3] = 0
        with pytest.raises(AssertionError, match=r"3 bytes before the start of tight workspace"):
            g.check()
    g.check()           # the production-like workspace is intact
    g.ws.raw[g.ws.lead + g.ws.nbytes + 5] = 1
    with pytest.raises(AssertionError, match=r"5 bytes past the end of workspace \(1048576 bytes\)"):
        g.check()


def test_write_into_a_persistent_buffers_leading_margin(gc):
    g, ctx = gc
    p = ctx.persistent((8,), L.F32, fill=1.0)
    q = ctx.persistent((3, 3), "i32")
    _bytes(q).zero_()
    g.check()
    _poke(q, -256)
    with pytest.raises(AssertionError, match=r"256 bytes before the start of persistent buffer #2 \(3, 3\) \(36 bytes\)"):
        g.check()
    g.forget_persistent()      # (still damaged) ... a forgotten frame no longer takes part
    g.check()


def test_unwritten_counts_elements_that_keep_the_fill(gc):
    g, ctx = gc
    for dt, tdt in ((L.F32, torch.float32), (L.BF16, torch.bfloat16), ("i32", torch.int32)):
        t = ctx.empty((5, 7), dt)
        assert g.unwritten(t) == 35
        v = _bytes(t).view(tdt)
        v[:] = 1
        assert g.unwritten(t) == 0
        _bytes(t)[t.itemsize * 11:t.itemsize * 12] = 0xFF
        assert g.unwritten(t) == 1
    p = ctx.persistent((6,), L.F32)
    assert g.unwritten(p) == 6
