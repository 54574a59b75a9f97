"""The graph-capture protocols of the host layer on their error paths: Context.capture, runtime.run_rehearsed (the rehearse-then-capture
protocol of CifarRCGAN._run and MnistRCGAN._run) and MnistRCGAN._run_once (run exactly once, no rehearsal).

The body of every case is one accumulating launch, acc += 1 over a persistent 256-float buffer (rcgan_axpby, an op the captured
production steps use), so the buffer's value counts how often the body was EXECUTED -- a capture records it without running it.  Every
exception is raised on the host by the test's own closure; no invalid launch is issued.  The engines' methods are driven with a stand-in
for ``self`` that carries the few attributes they read, so no model has to be built."""
import types
import warnings

import numpy as np
import pytest

from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

N = 256


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 24)
    yield c
    c.close()


class Counter:
    """bump(): the accumulating launch, then whatever ``then`` does on the host.  executed(): how often the launch has run."""

    def __init__(self, ctx, then=None):
        from rcgan_amd import _lib as L
        self.ctx, self.then, self.F32 = ctx, then, L.F32
        self.acc, self.ones = ctx.persistent((N,), L.F32, fill=0.0), ctx.persistent((N,), L.F32, fill=1.0)
        ctx.sync()

    def bump(self):
        c = self.ctx
        c.check(c.lib.rcgan_axpby(c.h, N, self.F32, 1.0, self.ones.ptr, 1.0, self.acc.ptr))
        if self.then is not None:
            self.then()

    def executed(self):
        a = self.ctx.download(self.acc)
        assert (a == a[0]).all(), a
        assert a[0] == int(a[0])
        return int(a[0])


def _raise(exc):
    raise exc


def _rccl_error():
    from rcgan_amd import _lib as L
    return L.RcganError(L.RCGAN_ERCCL, "made by the test on the host: a collective that cannot be recorded")


def test_capture_leaves_capture_mode_on_any_exception(ctx):
    bad = Counter(ctx, then=lambda: _raise(ValueError("after the launch")))
    with pytest.raises(ValueError, match="after the launch"):
        ctx.capture(bad.bump)
    assert not ctx.capturing
    assert bad.executed() == 0                  # recorded into a dropped capture, never run
    good = Counter(ctx)
    good.bump()                                 # the stream takes eager work again
    ctx.sync()
    assert good.executed() == 1
    gid = ctx.capture(good.bump, reserve=1 << 20)
    try:
        assert not ctx.capturing and good.executed() == 1
        for want in (2, 3):
            ctx.graph_launch(gid)
            ctx.sync()
            assert good.executed() == want
    finally:
        ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, gid))
    assert bad.executed() == 0


def test_rehearsed_protocol_executes_once_per_call(ctx):
    from rcgan_amd.mnist import MnistRCGAN
    from rcgan_amd.runtime import run_rehearsed
    k, graphs = Counter(ctx), {}
    for call in (1, 2, 3):                      # call 1: the eager run counts, its capture does not; calls 2, 3: one replay each
        run_rehearsed(graphs, "step", k.bump, ctx)
        assert k.executed() == call and not ctx.capturing
        assert list(graphs) == ["step"] and isinstance(graphs["step"], int)
    ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, graphs["step"]))
    for use_graphs in (True, False):            # the engine's method: the same with graphs, a plain call of the body without
        k, me = Counter(ctx), types.SimpleNamespace(ctx=ctx, use_graphs=use_graphs, _graphs={})
        for call in (1, 2, 3):
            MnistRCGAN._run(me, "step", k.bump)
            assert k.executed() == call
        assert list(me._graphs) == (["step"] if use_graphs else [])
        if use_graphs:
            ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, me._graphs["step"]))


def test_rehearsed_protocol_tolerated_error_runs_uncaptured_from_then_on(ctx):
    from rcgan_amd import _lib as L
    from rcgan_amd.cifar import CifarRCGAN
    from rcgan_amd.runtime import run_rehearsed
    refuse = lambda: _raise(_rccl_error()) if ctx.capturing else None
    k, graphs, seen = Counter(ctx, then=refuse), {}, []
    accept = lambda e: seen.append(e.code) or e.code == L.RCGAN_ERCCL
    for call in (1, 2, 3):
        run_rehearsed(graphs, "step", k.bump, ctx, accept)
        assert k.executed() == call and not ctx.capturing
        assert graphs == {"step": None}
    assert seen == [L.RCGAN_ERCCL]              # asked once, at the capture
    # a predicate that does not accept it, and none at all: the error travels on, nothing is stored, the stream is usable
    for predicate in (lambda e: False, None):
        k, graphs = Counter(ctx, then=refuse), {}
        with pytest.raises(L.RcganError, match="made by the test"):
            run_rehearsed(graphs, "step", k.bump, ctx, predicate)
        assert not ctx.capturing and graphs == {}
        assert k.executed() == 1                # the rehearsal
        k.bump()
        ctx.sync()
        assert k.executed() == 2
    # CifarRCGAN._run tolerates exactly this error under data parallel, with its warning, and not otherwise
    k, me = Counter(ctx, then=refuse), types.SimpleNamespace(ctx=ctx, use_graphs=True, _graphs={}, dp_active=True)
    with pytest.warns(UserWarning, match=r"step 'step': the all-reduce could not be captured \(.*\); running it uncaptured"):
        CifarRCGAN._run(me, "step", k.bump)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        CifarRCGAN._run(me, "step", k.bump)
    assert me._graphs == {"step": None} and k.executed() == 2
    me = types.SimpleNamespace(ctx=ctx, use_graphs=True, _graphs={}, dp_active=False)
    with pytest.raises(L.RcganError, match="made by the test"):
        CifarRCGAN._run(me, "step", k.bump)
    assert not ctx.capturing and me._graphs == {} and k.executed() == 3


def test_run_once_protocol_falls_back_to_one_eager_run_then_captures(ctx):
    from rcgan_amd import _lib as L
    from rcgan_amd.mnist import MnistRCGAN
    captured_runs = []

    def first_capture_fails():
        if ctx.capturing:
            captured_runs.append(1)
            if len(captured_runs) == 1:
                raise L.RcganError(L.RCGAN_EHIP, "made by the test on the host: scratch would have to grow")
    k, me = Counter(ctx, then=first_capture_fails), types.SimpleNamespace(ctx=ctx, use_graphs=True, _graphs={}, B=4)
    MnistRCGAN._run_once(me, "d_keep", k.bump)
    assert k.executed() == 1 and me._graphs == {} and not ctx.capturing        # dropped capture, one eager run as this step
    MnistRCGAN._run_once(me, "d_keep", k.bump)
    assert k.executed() == 2 and isinstance(me._graphs["d_keep"], int)          # captured and launched
    MnistRCGAN._run_once(me, "d_keep", k.bump)
    assert k.executed() == 3 and len(captured_runs) == 2                        # replayed: the body was not called again
    ctx.check(ctx.lib.rcgan_graph_destroy(ctx.h, me._graphs["d_keep"]))
    k, me = Counter(ctx), types.SimpleNamespace(ctx=ctx, use_graphs=False, _graphs={}, B=4)
    for call in (1, 2):
        MnistRCGAN._run_once(me, "d_keep", k.bump)
        assert k.executed() == call and me._graphs == {}
