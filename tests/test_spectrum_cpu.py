"""The radial power-spectrum distance without a GPU: the float64 restatement (tests/spectrum_ref.py) against closed forms, the
evaluator's host arithmetic on given spectra (a stub stands in for the two device calls), the orderings the numbers exist for on the
inputs the GPU test reuses, and the library's export and argument checks."""
import ctypes as C

import numpy as np
import pytest

import rcgan_amd  # noqa: F401
from rcgan_amd import _lib, spectrum
from tests import spectrum_ref as SR

COUNTS_32 = [1, 8, 12, 16, 32, 28, 40, 40, 48, 68, 56, 72, 68, 88, 88, 84, 94, 64, 44, 32, 16, 20, 4, 1]
COUNTS_9 = [1, 8, 12, 16, 32, 8, 4]


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N", [8, 9, 16, 28, 32])
def test_ring_tables(N):
    table, counts = SR.rings(N)
    got_table, got_counts = spectrum.rings(N)
    assert np.array_equal(got_table, table) and np.array_equal(got_counts, counts)
    assert counts.sum() == N * N and counts[0] == 1 and table[0, 0] == 0 and (counts > 0).all()
    assert len(counts) == {8: 7, 9: 7, 16: 12, 28: 21, 32: 24}[N]
    if N == 32:
        assert counts.tolist() == COUNTS_32
    if N == 9:
        assert counts.tolist() == COUNTS_9
    if N % 2 == 0:
        assert table[N // 2, N // 2] == len(counts) - 1 and counts[-1] == (5 if N == 16 else 1)   # the checkerboard point, alone at 8, 28, 32
        assert table[N // 2, 0] == N // 2 and table[0, N // 2] == N // 2              # the axis Nyquist points
    assert np.array_equal(table, table.T) and np.array_equal(table[1:], table[1:][::-1])   # f(u) and f(N - u) differ in sign only


@pytest.mark.parametrize("N", [9, 28, 32])
def test_an_impulse_has_a_flat_spectrum(N):
    x = np.full((2, N, N, 3), 128, np.uint8)
    x[0, 3, 5, :], x[1, N - 1, 0, :] = 128 + 90, 128 - 77
    S = SR.spectrum(x)
    assert np.abs(S[0] - 90.0 ** 2 / N ** 2).max() <= 1e-9 and np.abs(S[1] - 77.0 ** 2 / N ** 2).max() <= 1e-9


@pytest.mark.parametrize("N", [8, 28, 32])
def test_a_checkerboard_lives_on_the_last_ring_and_a_constant_on_ring_zero(N):
    y, x = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    board = (255 * ((y + x) % 2)).astype(np.uint8)[None, :, :, None]
    S = SR.spectrum(board)[0, 0]
    B = len(S)
    # a = +-127.5 - 0.5: the alternating part 127.5 sums to 127.5 N^2 at (N/2, N/2), the constant -0.5 sits on ring 0
    assert S[B - 1] == pytest.approx((255.0 * N * N / 2) ** 2 / N ** 2, rel=1e-12)
    assert np.abs(S[1:B - 1]).max() <= 1e-12 * S[B - 1]
    flat = SR.spectrum(np.full((1, N, N, 1), 200, np.uint8))[0, 0]
    assert flat[0] == pytest.approx((72.0 * N * N) ** 2 / N ** 2, rel=1e-12) and np.abs(flat[1:]).max() <= 1e-12 * flat[0]
    assert not SR.spectrum(np.full((1, N, N, 3), 128, np.uint8)).any()


@pytest.mark.parametrize("N, c", [(9, 1), (28, 1), (32, 3)])
def test_parseval(N, c):
    x = np.random.RandomState(N).randint(0, 256, size=(5, N, N, c)).astype(np.uint8)
    _, counts = SR.rings(N)
    energy = ((x.astype(np.float64) - 128) ** 2).sum(axis=(1, 2))
    assert np.allclose((SR.spectrum(x) * counts).sum(axis=2), energy, rtol=1e-12, atol=0)
    assert np.allclose((SR.spectrum_f32(x).astype(np.float64) * counts).sum(axis=2), energy, rtol=1e-5, atol=0)


def test_the_fp32_restatement_lies_within_the_bound_and_the_bound_is_not_vacuous():
    for N in (9, 28, 32):
        for name, x in SR.families(N, 3, 12).items():
            err, bound = np.abs(SR.spectrum_f32(x).astype(np.float64) - SR.spectrum(x)), SR.bound(x)
            assert (err <= 0.1 * bound).all(), (N, name)
    x = SR.families(32, 3, 12)["uniform"]
    S, b = SR.spectrum(x), SR.bound(x)
    assert (b[..., 1:-1] <= 1e-2 * S[..., 1:-1]).all()
    assert (b.mean(axis=(0, 1))[1:] <= 1e-2 * S.mean(axis=(0, 1))[1:]).all()


# ------------------------------------------------------------------------------------------------------------------ the evaluator on a stub
class Stub:
    """Stands in for the two device calls: image i carries its spectrum's row number in its first two pixels."""

    def __init__(self, monkeypatch, table=None):
        self.table, self.calls = table, dict(image_spectra=0, class_sums=0)
        monkeypatch.setattr(spectrum, "image_spectra", self.image_spectra)
        monkeypatch.setattr(spectrum, "class_sums", self.class_sums)

    def image_spectra(self, ctx, x):
        self.calls["image_spectra"] += 1
        if self.table is None:
            return SR.spectrum(x).reshape(len(x), -1)
        return self.table[x[:, 0, 0, 0].astype(int) * 256 + x[:, 0, 1, 0]].reshape(len(x), -1)

    def class_sums(self, ctx, rows, labels, n_classes):
        self.calls["class_sums"] += 1
        count, total = np.zeros(n_classes), np.zeros((n_classes, rows.shape[1]))
        for k in range(n_classes):
            count[k], total[k] = (labels == k).sum(), rows[labels == k].sum(axis=0)
        return count, total


def carriers(rows, N=16):
    x = np.zeros((len(rows), N, N, 1), np.uint8)
    x[:, 0, 0, 0], x[:, 0, 1, 0] = np.asarray(rows) // 256, np.asarray(rows) % 256
    return x


def test_dropped_rings_undefined_and_left_out_classes_and_the_standard_error(monkeypatch):
    N, K = 16, 5
    _, counts = SR.rings(N)
    B = len(counts)
    rs = np.random.RandomState(0)
    table = np.exp(rs.randn(60, 1, B))                                # 60 spectra, rows 0..29 real, 30..59 generated
    real_labels = np.repeat(np.arange(K), 6)                          # 6 real images per class
    labels = np.array([0] * 6 + [1] * 6 + [2] * 6 + [3] * 1 + [4] * 6 + [7] * 5)   # class 3: one image; five foreign labels
    table[30:36, 0, 5] = 0.0                                          # class 0: ring 5 has no energy on the generated side
    table[12:18, 0, :] = 0.0                                          # class 2: the real side has no energy at all
    Stub(monkeypatch, table)
    ev = spectrum.SpectrumEvaluator(K, ctx=object())
    assert ev.prepare_real(carriers(np.arange(30)), real_labels)["rows"].tolist() == [6] * K
    r = ev.evaluate(carriers(30 + np.arange(30)), labels)
    assert r["left_out"] == [3] and r["undefined"] == [2] and r["classes_used"] == 3 and r["rejected_generated"] == 5
    per = r["per_class_spectral_distance"]
    assert np.isnan(per[[2, 3]]).all() and not np.isnan(per[[0, 1, 4]]).any()
    # class 0 by hand: ring 5 is dropped from the mean, the other rings b >= 1 count
    g, rr = table[30:36, 0].mean(axis=0), table[0:6, 0].mean(axis=0)
    keep = [b for b in range(1, B) if b != 5]
    assert per[0] == pytest.approx(np.sqrt(np.mean((10 * np.log10(g[keep] / rr[keep])) ** 2)), rel=1e-12)
    assert r["per_class_nyquist_db"][0] == pytest.approx(10 * np.log10(g[N // 2] / rr[N // 2]), rel=1e-12)
    assert r["per_class_checkerboard_db"][0] == pytest.approx(10 * np.log10(g[B - 1] / rr[B - 1]), rel=1e-12)
    hf = lambda s: (counts[5:] * s[5:]).sum() / (counts[1:] * s[1:]).sum()                # b > N / 4 = 4
    assert r["per_class_high_frequency_db"][0] == pytest.approx(10 * np.log10(hf(g) / hf(rr)), rel=1e-12)
    used = per[[0, 1, 4]]
    assert r["intra_class_spectral_distance"] == pytest.approx(used.mean(), rel=1e-14)
    assert r["intra_class_spectral_distance_se"] == pytest.approx(used.std(ddof=1) / np.sqrt(3), rel=1e-12)
    assert r["intra_class_nyquist_db"] == pytest.approx(r["per_class_nyquist_db"][[0, 1, 4]].mean(), rel=1e-12)
    # the pooled value: every kept image of each side, the zero rows of real class 2 included in the mean
    want = SR.compare(table[30:55].mean(axis=0), table[0:30].mean(axis=0), N)
    for name in SR.NAMES:
        assert r[name] == pytest.approx(want[name], rel=1e-12), name
    # and the whole result against the restatement fed the same spectra
    ref = SR.evaluate(carriers(np.arange(30)), real_labels, carriers(30 + np.arange(30)), labels, K,
                      spectrum_fn=lambda x: table[x[:, 0, 0, 0].astype(int) * 256 + x[:, 0, 1, 0]])
    assert SR.relative_difference(ref, r) <= 1e-12
    curves = ev.spectra()
    assert curves["real"].shape == (1, B) and curves["generated_per_class"].shape == (K, 1, B)
    assert np.allclose(curves["generated_per_class"][0, 0], g, rtol=1e-14) and curves["ring_counts"].tolist() == counts.tolist()
    ev.close()


def test_floors_are_kept_per_count_vector(monkeypatch):
    w = SR.world(3, 8, 16, 1, seed=3)
    stub = Stub(monkeypatch)
    ev = spectrum.SpectrumEvaluator(3, ctx=object())
    ev.prepare_real(w["real"], w["real_labels"])
    first = ev.evaluate(w["fresh"], w["labels"])
    calls = dict(stub.calls)
    second = ev.evaluate(w["blurred"], w["labels"])
    assert stub.calls["class_sums"] - calls["class_sums"] == 1 and stub.calls["image_spectra"] - calls["image_spectra"] == 1
    assert len(ev.floors) == 1 and second["floor_spectral_distance"] == first["floor_spectral_distance"]
    assert np.array_equal(second["floor_per_class_spectral_distance"], first["floor_per_class_spectral_distance"])
    ref = SR.evaluate(w["real"], w["real_labels"], w["fresh"], w["labels"], 3)
    assert SR.relative_difference(ref, first) <= 1e-12                 # floors included: rows [0, m') against [m', 2 m') per class
    fewer = w["labels"].copy()
    fewer[np.flatnonzero(fewer == 1)[:5]] = -1                         # another count vector: another floor
    third = ev.evaluate(w["fresh"], fewer)
    assert len(ev.floors) == 2 and stub.calls["class_sums"] - calls["class_sums"] == 1 + 4          # the set, then a pooled and two per-class floor calls
    assert SR.relative_difference(SR.evaluate(w["real"], w["real_labels"], w["fresh"], fewer, 3), third) <= 1e-12
    ev.close()


def test_the_orderings_hold_in_the_restatement():
    K = 4
    w = SR.world(K, 40, 32, 3)
    ev = lambda x: SR.evaluate(w["real"], w["real_labels"], x, w["labels"], K)
    res = {name: ev(w[name]) for name in ("fresh", "blurred", "checker", "striped")}
    for name, r in res.items():
        print("%-8s %s floor %.3f intra-class %.3f floor %.3f" % (name, {n: round(r[n], 2) for n in SR.NAMES}, r["floor_spectral_distance"],
                                                               r["intra_class_spectral_distance"], r["floor_intra_class_spectral_distance"]))
    SR.orderings(res["fresh"]["floor_spectral_distance"], res["fresh"], res["blurred"], res["checker"], res["striped"])
    per = {name: dict((n, r["intra_class_" + n]) for n in SR.NAMES) for name, r in res.items()}
    SR.orderings(res["fresh"]["floor_intra_class_spectral_distance"], per["fresh"], per["blurred"], per["checker"], per["striped"])


def test_image_layouts_and_bad_sets_are_told_apart(monkeypatch):
    Stub(monkeypatch)
    ev = spectrum.SpectrumEvaluator(2, ctx=object())
    rs = np.random.RandomState(1)
    mnist = rs.randint(0, 256, size=(8, 784))
    assert ev.prepare_real(mnist, np.arange(8) % 2)["images"] == 8 and ev.real["shape"] == (28, 28, 1)
    with pytest.raises(ValueError):
        ev.evaluate(rs.randint(0, 256, size=(8, 3072)), np.arange(8) % 2)          # CIFAR rows against an MNIST real set
    with pytest.raises(ValueError):
        spectrum.as_images(np.zeros((2, 28, 32, 1), np.uint8))                    # not square
    with pytest.raises(RuntimeError):
        spectrum.SpectrumEvaluator(2, ctx=object()).evaluate(mnist, np.arange(8) % 2)
    ev.close()


# ------------------------------------------------------------------------------------------------------------------ the library
def test_the_library_exports_the_call_and_refuses_it_without_a_context():
    lib = _lib.load()
    assert "rcgan_radial_spectrum" in _lib.SIGNATURES and hasattr(lib, "rcgan_radial_spectrum") and hasattr(_lib.load("f16"), "rcgan_radial_spectrum")
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    for n, N, c, x, out in ((1, 32, 3, p, p), (1, 7, 3, p, p), (1, 33, 3, p, p), (1, 32, 2, p, p), (1, 32, 4, p, p), (0, 32, 3, p, p),
                            (-1, 32, 3, p, p), (1, 32, 3, None, p), (1, 32, 3, p, None)):
        assert lib.rcgan_radial_spectrum(None, n, N, c, x, out) == _lib.EINVALID_ARG, (n, N, c)
