"""Guard bands around everything a kernel may write: a checker for memory safety where no device sanitizer can run.

``guarded(ctx)`` swaps four attributes of ONE ``Context`` instance -- ``arena``, ``persistent``, ``ws_ptr`` and ``ws_bytes`` -- for
versions that frame every allocation with margins of 0xFF bytes, and restores them on exit:

  arena      : every ``alloc`` gets >= 64 KiB in front of and behind its body; buffer, margins and bodies start out as 0xFF (a NaN as
               fp32, bf16 and fp16, -1 as int32), so an input's neighbourhood is poison and an output that was never written shows.
  persistent : body + two margins inside one torch tensor that stays alive (FakeParam values and gradients, moving statistics, losses).
  workspace  : 256 MiB framed by 1 MiB margins, or -- inside ``with g.workspace(nbytes)`` -- a region of EXACTLY ``nbytes`` (start rounded
               to 256 bytes) framed the same way: the size a caller who trusts a ``*_workspace_bytes`` function would pass.

``g.check()`` (after ``ctx.sync()``) asserts that every byte outside the bodies is still 0xFF and names the allocation and the offset of the
first byte that is not; the arena's ``reset()`` (``Context.new_step``) checks too before it refills.  ``g.unwritten(t)`` counts the elements of a tensor that still hold the fill pattern.

A limit to keep in mind: ``alloc`` refills the margins and the body of the NEW allocation, so a stray write that landed beyond an earlier
allocation's 64 KiB trailing margin is erased when the next tensor is allocated over that place before ``check()`` runs.  Writes within the
margins are always seen; "space that was never allocated" is only the space behind the LAST allocation of a step.

Everything is torch on raw ``uint8`` views of the given device, so the same code runs on ``torch.device("cpu")`` with a stub in place
of the Context (tests/test_guard_cpu.py): a check costs milliseconds.
"""
import contextlib

import torch

ALIGN = 256
FILL = 0xFF
MARGIN = 64 << 10           # arena / persistent margins (a multiple of ALIGN)
WS_MARGIN = 1 << 20         # workspace margins
SLACK = 1 << 20             # arena bytes checked (and refilled) past the high-water mark: space that was never allocated
WS_DEFAULT = 256 << 20      # the production-like workspace


def _round_up(v, a=ALIGN):
    return (int(v) + a - 1) // a * a


def _first_bad(raw, lo, hi):
    """Offset of the first byte of raw[lo:hi] that is not FILL (the range is known to hold one)."""
    step = 1 << 24
    for a in range(lo, hi, step):
        bad = torch.nonzero(raw[a:min(hi, a + step)] != FILL)
        if bad.numel():
            return a + int(bad[0, 0])
    raise AssertionError("no damaged byte in [%d, %d)" % (lo, hi))


class GuardedArena:
    """The interface of runtime.Arena (buf, base, cap, off, peak, reset, alloc) with a margin on both sides of every body."""

    def __init__(self, guard, nbytes):
        self.g = guard
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=guard.device)
        self.base = self.buf.data_ptr()
        self.cap = int(nbytes)
        self.off = 0
        self.peak = 0
        self.bodies = []        # (start, end) offsets of the bodies handed out since the last reset, ascending
        with guard.on_stream():
            self.buf.fill_(FILL)

    def checked_end(self):
        return min(self.cap, self.peak + SLACK)

    def reset(self):
        """Context.new_step(): check first -- a test body that takes several steps must not wipe unseen what the last one damaged."""
        self.g.settle()
        self.g.check()
        self.wipe()

    def wipe(self):
        with self.g.on_stream():
            self.buf[:self.checked_end()].fill_(FILL)
        self.off = 0
        self.bodies = []
        self.g.refill_workspace()

    def alloc(self, nbytes):
        nbytes = int(nbytes)
        off = _round_up(self.base + self.off) - self.base           # (absolute alignment: a host buffer need not start on ALIGN)
        body = off + MARGIN
        end = body + nbytes + MARGIN
        if end > self.cap:
            raise MemoryError("guarded arena exhausted: need %d more bytes (capacity %d)" % (end - self.cap, self.cap))
        with self.g.on_stream():
            self.buf[off:end].fill_(FILL)
        self.g.settle()
        self.bodies.append((body, body + nbytes))
        self.off = end
        self.peak = max(self.peak, self.off)
        return self.base + body

    def gaps(self):
        """(lo, hi, body in front or None, body behind or None) of every stretch outside the bodies, up to the checked end."""
        out, lo, prev = [], 0, None
        for k, (a, b) in enumerate(self.bodies):
            out.append((lo, a, prev, k))
            lo, prev = b, k
        out.append((lo, self.checked_end(), prev, None))
        return out

    def describe(self, off, before, after):
        name = lambda k: "arena allocation #%d (offset %d, %d bytes)" % (k, self.bodies[k][0], self.bodies[k][1] - self.bodies[k][0])
        if before is not None and off < self.bodies[before][1] + MARGIN:
            return "%d bytes past the end of %s" % (off - self.bodies[before][1], name(before))
        if after is not None and off >= self.bodies[after][0] - MARGIN:
            return "%d bytes before the start of %s" % (self.bodies[after][0] - off, name(after))
        if before is not None:
            return "%d bytes past the end of %s, in space that was never allocated" % (off - self.bodies[before][1], name(before))
        return "arena offset %d, in space that was never allocated" % off


class _Frame:
    """A body between two margins inside one torch tensor (persistent buffers, workspaces)."""

    def __init__(self, guard, nbytes, margin, name):
        self.name, self.nbytes, self.margin = name, int(nbytes), margin
        self.raw = torch.empty(margin + ALIGN + self.nbytes + margin, dtype=torch.uint8, device=guard.device)
        self.lead = margin + (-(self.raw.data_ptr() + margin)) % ALIGN          # body start rounded up to ALIGN
        self.ptr = self.raw.data_ptr() + self.lead
        with guard.on_stream():
            self.raw.fill_(FILL)

    def body(self):
        return self.raw[self.lead:self.lead + self.nbytes]

    def gaps(self):
        return [(0, self.lead, "before the start"), (self.lead + self.nbytes, self.raw.numel(), "past the end")]


class Guard:
    def __init__(self, ctx, device=None, arena_bytes=1 << 30, ws_bytes=WS_DEFAULT):
        self.ctx = ctx
        self.device = torch.device(device) if device is not None else ctx.device
        self.cuda = self.device.type == "cuda"
        self.arena = GuardedArena(self, arena_bytes)
        self.frames = []                  # persistent buffers since the last forget_persistent()
        self.n_persistent = 0
        self.ws_default = _Frame(self, ws_bytes, WS_MARGIN, "workspace (%d bytes)" % ws_bytes)
        self.ws = self.ws_default
        self._saved = None

    # ------------------------------------------------------------------ plumbing
    def on_stream(self):
        return torch.cuda.stream(self.ctx.stream) if self.cuda else contextlib.nullcontext()

    def settle(self):
        """Fills run on ctx.stream; host code that then writes through torch's current stream (FakeParam, ctx.view(t).copy_) must find
        them finished.  Never inside a graph capture."""
        if self.cuda and not getattr(self.ctx, "capturing", False):
            self.ctx.stream.synchronize()

    def install(self):
        c = self.ctx
        self._saved = {k: c.__dict__.get(k, None) for k in ("arena", "ws_ptr", "ws_bytes")}
        self._had_persistent = "persistent" in c.__dict__
        self._old_persistent = c.__dict__.get("persistent")
        c.arena = self.arena
        c.persistent = self.persistent
        self._point(self.ws_default)
        return self

    def remove(self):
        c = self.ctx
        for k, v in self._saved.items():
            setattr(c, k, v)
        if self._had_persistent:
            c.persistent = self._old_persistent
        else:
            del c.__dict__["persistent"]
        self._saved = None

    def _point(self, frame):
        self.ws = frame
        self.ctx.ws_ptr, self.ctx.ws_bytes = frame.ptr, frame.nbytes

    # ------------------------------------------------------------------ persistent buffers
    def persistent(self, shape, dtype=None, fill=None):
        """Context.persistent inside a frame.  dtype: the _lib codes of the original (F32 by default)."""
        from rcgan_amd import _lib as L
        from rcgan_amd.runtime import DT
        dtype = L.F32 if dtype is None else dtype
        tdt = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16, "i32": torch.int32}[dtype]
        shape = tuple(int(s) for s in shape)
        t = DT(0, shape, dtype)
        nbytes = max(t.size, 1) * t.itemsize
        self.n_persistent += 1
        fr = _Frame(self, nbytes, MARGIN, "persistent buffer #%d %s (%d bytes)" % (self.n_persistent, shape, nbytes))
        if fill is not None:
            with self.on_stream():
                fr.body().view(tdt).fill_(fill)
        self.settle()
        self.frames.append(fr)
        t.ptr, t.base = fr.ptr, fr.raw
        return t

    def forget_persistent(self):
        """Drop the frames checked so far from later checks (their tensors live on while a DT refers to them)."""
        self.frames = []

    def clear(self):
        """A fresh start without a check (the beginning of a test: whatever an earlier, failed one left is not this one's finding)."""
        self.forget_persistent()
        self.arena.wipe()

    # ------------------------------------------------------------------ workspace
    def refill_workspace(self):
        with self.on_stream():
            self.ws.raw.fill_(FILL)

    @contextlib.contextmanager
    def workspace(self, nbytes):
        """ctx.ws_ptr / ctx.ws_bytes = a region of exactly nbytes between two 1 MiB margins, all of it 0xFF."""
        fr = _Frame(self, nbytes, WS_MARGIN, "tight workspace (%d bytes)" % int(nbytes))
        self.settle()
        self._point(fr)
        try:
            yield fr
        finally:
            self._point(self.ws_default)

    # ------------------------------------------------------------------ checks
    def check(self):
        """Every byte outside the bodies is still 0xFF: arena (offset 0 to the high-water mark + 1 MiB), both margins of every persistent
        buffer, both workspace margins (the active one and the production-like one).  Call after ctx.sync()."""
        jobs = []           # (raw bytes, lo, hi, describe(offset) -> str)
        ar = self.arena
        for lo, hi, before, after in ar.gaps():
            if hi > lo:
                jobs.append((ar.buf, lo, hi, lambda off, b=before, a=after: ar.describe(off, b, a)))
        frames = list(self.frames) + [self.ws_default] + ([self.ws] if self.ws is not self.ws_default else [])
        for fr in frames:
            for lo, hi, side in fr.gaps():
                edge = fr.lead if side == "before the start" else fr.lead + fr.nbytes
                jobs.append((fr.raw, lo, hi, lambda off, f=fr, s=side, e=edge: "%d bytes %s of %s%s" % (
                    e - off if s == "before the start" else off - e, s, f.name,
                    " (workspace byte %d)" % (off - f.lead) if "workspace" in f.name else "")))
        with self.on_stream():
            flags = torch.stack([(raw[lo:hi] != FILL).any() for raw, lo, hi, _ in jobs]).cpu()
            for ok, (raw, lo, hi, describe) in zip((~flags).tolist(), jobs):
                if not ok:
                    off = _first_bad(raw, lo, hi)
                    raise AssertionError("guard band damaged: first byte %s; value 0x%02x" % (describe(off), int(raw[off])))

    def unwritten(self, t):
        """How many elements of the device tensor t (a DT) still hold the fill pattern."""
        off = t.ptr - t.base.data_ptr()
        raw = t.base.view(torch.uint8).reshape(-1)[off:off + t.nbytes]
        with self.on_stream():
            if t.itemsize == 1:
                return int((raw == FILL).sum())
            return int((raw.view(torch.int16 if t.itemsize == 2 else torch.int32) == -1).sum())


@contextlib.contextmanager
def guarded(ctx, device=None, arena_bytes=1 << 30, ws_bytes=WS_DEFAULT):
    """Replace ctx.arena, ctx.persistent, ctx.ws_ptr and ctx.ws_bytes on this instance; restore them on exit.  Yields the Guard."""
    g = Guard(ctx, device, arena_bytes, ws_bytes).install()
    try:
        yield g
    finally:
        g.remove()
