"""The radial power spectrum on the GPU (csrc/spectrum.hip, rcgan_amd/spectrum.py) against the float64 restatement
(tests/spectrum_ref.py).

The kernel is compared under the bound DERIVED in the header of csrc/spectrum.hip (``spectrum_ref.bound`` restates it; nothing is
tuned): worst error / bound <= 1 on every image, channel and ring.  The evaluator is compared key by key to a relative tolerance
that was measured without the kernel: ten times the largest relative difference between the float64 restatement and its fp32
restatement of the same evaluator on the same inputs (2.83e-6 at 4 x 40 images of 32 x 32 x 3, 1.14e-5 at 2 x 30 of 28 x 28 x 1).

On "the bound is not vacuous": at even N ring B-1 is the single real value F(N/2, N/2) of an image, which for random pixels is
Gaussian around 0, so an individual image's bound / value there is 2 delta / |F| with no upper limit (above 1e-2 for about one
image in forty, in the restatement alone).  The cap of 1e-2 is therefore asserted per image on every ring 1..B-2, and on every ring
1..B-1 for the family as a whole (mean bound / mean value)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import spectrum_ref as SR
from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

RTOL_32 = 2.9e-5            # 10 x 2.83e-6, measured as the module's header says
RTOL_28 = 1.2e-4            # 10 x 1.14e-5
SIZES = (1, 3, 67)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 20)
    yield c
    c.close()


def dev(ctx, a):
    with torch.cuda.stream(ctx.stream):
        return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def run(ctx, x):
    from rcgan_amd import spectrum
    return spectrum.download(ctx, spectrum.radial_spectrum(ctx, dev(ctx, x))).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("N", [8, 9, 28, 32])
def test_every_family_lies_within_the_derived_bound(ctx, N, c):
    worst = {}
    for name, x in SR.families(N, c, max(SIZES)).items():
        want, bound = SR.spectrum(x), SR.bound(x)
        for n in SIZES:
            got = run(ctx, x[:n])
            assert got.shape == want[:n].shape
            err = np.abs(got - want[:n])
            ratio = float((err / bound[:n]).max()) if name != "constant_128" else float(err.max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert (err <= bound[:n]).all(), (name, n, ratio)
        if name == "constant_128":
            assert not got.any()                                                   # a = 0: exact zeros
        if name == "uniform":                                                      # the bound says something
            B = want.shape[2]
            assert (bound[..., 1:B - 1] <= 1e-2 * want[..., 1:B - 1]).all()
            assert (bound.mean(axis=(0, 1))[1:] <= 1e-2 * want.mean(axis=(0, 1))[1:]).all()
    print("N %d c %d: error / bound at most %s" % (N, c, {k: float("%.3g" % v) for k, v in worst.items()}))


def test_a_batch_larger_than_any_grid(ctx):
    fam = SR.families(32, 3, 683, seed=9)                                          # 3 x 683 = 2049
    x = np.concatenate([fam["mixed"], fam["uniform"], fam["blurred_noise"]])
    assert len(x) == 2049
    got, want, bound = run(ctx, x), SR.spectrum(x), SR.bound(x)
    err = np.abs(got - want)
    print("n 2049: error / bound at most %.3g" % (err / bound).max())
    assert (err <= bound).all()
    _, counts = SR.rings(32)
    energy = ((x.astype(np.float64) - 128) ** 2).sum(axis=(1, 2))
    assert np.allclose((got * counts).sum(axis=2), energy, rtol=1e-5, atol=1e-3)   # Parseval on the device's numbers


def test_closed_forms_and_no_leak_from_the_padding(ctx):
    for N in (28, 32):
        fam = SR.families(N, 3, 4)
        board, imp = fam["checkerboard"], fam["impulse"]
        got_b, got_i = run(ctx, board), run(ctx, imp)
        B = got_b.shape[2]
        # the board is 255 on even squares: a = +-127.5 - 0.5; ring B-1 holds (127.5 N^2)^2 / N^2, ring 0 (0.5 N^2)^2 / N^2
        assert np.allclose(got_b[..., B - 1], (127.5 * N * N) ** 2 / N ** 2, rtol=1e-5, atol=0)
        assert (np.abs(got_b[..., 1:B - 1]) <= SR.bound(board)[..., 1:B - 1]).all()
        for i in range(4):
            v = float(imp[i].astype(np.int64).max() if imp[i].max() != 128 else imp[i].min()) - 128.0
            assert (np.abs(got_i[i] - v * v / N ** 2) <= SR.bound(imp[i:i + 1])[0] + 1e-12).all()
    # an image of 28 pixels a side is its own transform: against the restatement at 28, which differs from a padded 32
    x = SR.families(28, 1, 5)["blurred_noise"]
    padded = np.full((5, 32, 32, 1), 128, np.uint8)
    padded[:, :28, :28] = x
    got, at32 = run(ctx, x), run(ctx, padded)
    assert got.shape == (5, 1, 21) and at32.shape == (5, 1, 24)
    assert (np.abs(got - SR.spectrum(x)) <= SR.bound(x)).all()
    assert np.abs(at32[..., :21] * (32 * 32) / (28 * 28) - got).max() > 1e3 * SR.bound(x).max()


def test_the_same_bits_eager_and_replayed_and_nothing_outside_the_tensors_is_touched(ctx):
    from rcgan_amd import spectrum
    n, N, c, B = 37, 32, 3, 24
    x = SR.families(N, c, n, seed=4)["mixed"]
    for lead in (16, 13):                                                          # 16-byte loads, then the byte path
        big = np.full(lead + x.size + 64, 0xFF, np.uint8)
        big[lead:lead + x.size] = x.reshape(-1)
        dbig = dev(ctx, big)
        dx = dbig[lead:lead + x.size].view(n, N, N, c)
        with torch.cuda.stream(ctx.stream):
            outs = [torch.full((n * c * B + 128,), float("nan"), dtype=torch.float32, device=dbig.device).view(torch.int32).fill_(-1).view(torch.float32)
                    for _ in range(3)]
        mid = lambda o: o[64:64 + n * c * B].view(n, c, B)
        spectrum.radial_spectrum(ctx, dx, out=mid(outs[0]))
        spectrum.radial_spectrum(ctx, dx, out=mid(outs[1]))
        ctx.stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=ctx.stream):                           # one stream, no parallel branches
            spectrum.radial_spectrum(ctx, dx, out=mid(outs[2]))
        ctx.stream.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = [o.view(torch.int32).cpu().numpy() for o in outs]
        for h in host:
            assert (h[:64] == -1).all() and (h[64 + n * c * B:] == -1).all()        # the margins of out
        assert host[0].tobytes() == host[1].tobytes() == host[2].tobytes()
        assert np.array_equal(dbig.cpu().numpy(), big)                             # x and its margins
        got = host[0][64:64 + n * c * B].view(np.float32).reshape(n, c, B).astype(np.float64)
        assert (np.abs(got - SR.spectrum(x)) <= SR.bound(x)).all()
        del graph


def test_bad_arguments_are_refused_before_any_launch(ctx):
    from rcgan_amd import _lib
    t = dev(ctx, np.zeros(4096, np.float32))
    p = C.c_void_p(t.data_ptr())
    f = ctx.lib.rcgan_radial_spectrum
    for n, N, c, x, out in ((1, 7, 3, p, p), (1, 33, 3, p, p), (1, 32, 2, p, p), (0, 32, 3, p, p), (1, 32, 3, None, p), (1, 32, 3, p, None)):
        assert f(ctx.h, n, N, c, x, out) == _lib.EINVALID_ARG
    assert not spectrum_download(ctx, t).any()


def spectrum_download(ctx, t):
    from rcgan_amd import spectrum
    return spectrum.download(ctx, t)


# ------------------------------------------------------------------------------------------------------------------ end to end
def counted(monkeypatch, spectrum):
    calls = dict(radial_spectrum=0, class_sums=0)
    for name in calls:
        def wrap(*a, _f=getattr(spectrum, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(spectrum, name, wrap)
    return calls


@pytest.mark.parametrize("K, per_class, N, c, rtol", [(4, 40, 32, 3, RTOL_32), (2, 30, 28, 1, RTOL_28)])
def test_the_evaluator_agrees_with_the_restatement_key_by_key(monkeypatch, K, per_class, N, c, rtol):
    from rcgan_amd import spectrum
    w = SR.world(K, per_class, N, c)
    calls = counted(monkeypatch, spectrum)
    ev = spectrum.SpectrumEvaluator(K)
    try:
        ev.prepare_real(w["real"], w["real_labels"])
        got = {name: ev.evaluate(w[name], w["labels"]) for name in ("fresh", "blurred", "checker", "striped")}
        assert calls == dict(radial_spectrum=5, class_sums=1 + 4 + 3) and len(ev.floors) == 1      # the floor: computed once, then kept
        for name, r in got.items():
            ref = SR.evaluate(w["real"], w["real_labels"], w[name], w["labels"], K)
            diff = SR.relative_difference(ref, r)
            print("%d x %d at %d x %d x %d, %-8s: largest relative difference %.3g (tolerance %.3g)" % (K, per_class, N, N, c, name, diff, rtol))
            assert diff <= rtol, name
            assert r["classes_used"] == K and r["left_out"] == [] and r["undefined"] == []
        SR.orderings(got["fresh"]["floor_spectral_distance"], got["fresh"], got["blurred"], got["checker"], got["striped"])
        curves = ev.spectra()
        assert curves["generated_per_class"].shape == (K, c, len(SR.rings(N)[1]))
        assert np.allclose(curves["real"], SR.spectrum(w["real"]).mean(axis=0), rtol=1e-5)
        # one class emptied on the generated side
        labels = w["labels"].copy()
        labels[labels == 1] = K + 3
        r = ev.evaluate(w["fresh"], labels)
        assert r["left_out"] == [1] and r["classes_used"] == K - 1 and np.isnan(r["per_class_spectral_distance"][1]) and r["rejected_generated"] == per_class
        assert SR.relative_difference(SR.evaluate(w["real"], w["real_labels"], w["fresh"], labels, K), r) <= rtol
        assert len(ev.floors) == 2
        json.dumps(spectrum.json_ready(r))
    finally:
        ev.close()


def test_the_stand_alone_tool_prints_the_in_process_value(tmp_path):
    from rcgan_amd import spectrum
    w = SR.world(2, 12, 32, 3, seed=8)
    a, b = os.path.join(str(tmp_path), "real.npz"), os.path.join(str(tmp_path), "generated.npz")
    np.savez(a, images=w["real"], labels=w["real_labels"])
    np.savez(b, images=w["checker"].transpose(0, 3, 1, 2).reshape(-1, 3072), labels=w["labels"])          # (both layouts are taken)
    ev = spectrum.SpectrumEvaluator(2)
    try:
        ev.prepare_real(w["real"], w["real_labels"])
        want = ev.evaluate(w["checker"], w["labels"])
    finally:
        ev.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, "-m", "rcgan_amd.spectrum", "--real", a, "--generated", b], cwd=root, capture_output=True, text=True,
                           timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    line = [l for l in child.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    assert r["spectral_distance"] == want["spectral_distance"] and r["checkerboard_db"] == want["checkerboard_db"]
    assert r["floor_spectral_distance"] == want["floor_spectral_distance"] and r["classes_used"] == 2


def test_the_schedule_runs_the_metric_on_a_numpy_sampler_and_writes_the_curves(tmp_path, caplog):
    import logging
    from rcgan_amd import metrics, train_cifar
    from rcgan_amd.cifar import Z_DIM
    FLAGS = train_cifar.define_flags().parse(["--spectrum_freq", "2", "--spectrum_samples", "200", "--spectrum_real_samples", "400"])
    metrics.check_flags(FLAGS)
    rs = np.random.RandomState(2)
    rows = lambda n: SR.quantise(SR.blurred_noise(rs, n, 32, 3)).transpose(0, 3, 1, 2).reshape(-1, 3072)
    train = (rows(500), np.arange(500) % 10)
    sample = lambda labels, z: rows(len(labels)) / 127.5 - 1.0
    plotted = []
    plot = type("Plot", (), dict(plot=staticmethod(lambda name, value: plotted.append((name, value)))))
    caplog.set_level(logging.INFO)
    E = metrics.Evaluations(FLAGS, 10, 0, str(tmp_path), sample, np.random.RandomState(3), plot, np.zeros((100, Z_DIM), np.float32),
                            train_cifar.grid_labels(10), lambda: train, lambda: None)
    for iteration in range(2):
        E.run(iteration)
    E.close()
    lines = [r.getMessage() for r in caplog.records]
    assert [l for l in lines if "calculating" in l] == ["starting calculating radial power spectrum.", "finished calculating radial power spectrum."]
    assert "spectrum real set: 400 images" in lines
    assert sum(l.startswith("intra_class_spectral_distance: ") and "(10 of 10 classes), floor " in l for l in lines) == 1
    assert [n for n, _ in plotted] == ["spectral_distance", "floor_spectral_distance", "intra_class_spectral_distance",
                                      "floor_intra_class_spectral_distance", "high_frequency_db", "nyquist_db", "checkerboard_db"]
    assert all(np.isfinite(v) for _, v in plotted) and plotted[0][1] > 0
    with np.load(os.path.join(str(tmp_path), "spectrum_1.npz")) as z:
        assert z["real"].shape == (3, 24) and z["generated_per_class"].shape == (10, 3, 24) and z["ring_counts"].sum() == 1024
        assert (z["generated"] > 0).all()
