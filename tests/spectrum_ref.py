"""The radial power-spectrum distance restated in float64 numpy (the yardstick of rcgan_amd/spectrum.py and csrc/spectrum.hip), the
bound of the kernel's header, a float32 restatement of the kernel's arithmetic, and the image families the tests share.

Written from the definition, not from the product: explicit DFT matrices with the index product reduced mod N before the angle, loops
over classes, no code shared with rcgan_amd/spectrum.py."""
import numpy as np

U = 2.0 ** -24


def signed(N):
    return np.array([u if u <= N // 2 else u - N for u in range(N)], dtype=np.int64)


def ring_of(fu, fv):
    """The b with (2b - 1)^2 <= 4 (fu^2 + fv^2) < (2b + 1)^2, by counting up: integers only."""
    r2 = 4 * (int(fu) ** 2 + int(fv) ** 2)
    b = 0
    while (2 * b + 1) ** 2 <= r2:
        b += 1
    assert b == 0 or (2 * b - 1) ** 2 <= r2 < (2 * b + 1) ** 2
    return b


def rings(N):
    f = signed(N)
    table = np.array([[ring_of(f[u], f[v]) for v in range(N)] for u in range(N)], dtype=np.int64)
    return table, np.bincount(table.reshape(-1))


def twiddles(N, dtype=np.float64):
    k = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N
    ang = 2.0 * np.pi * k.astype(np.float64) / N
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


def transform(x, dtype=np.float64):
    """uint8 [n,N,N,c] -> (Re F, Im F), each [n,c,N,N] (u, v), in ``dtype``: A C then C (.) - the two-pass form of the kernel."""
    x = np.asarray(x)
    N = x.shape[1]
    a = (x.astype(np.int64) - 128).transpose(0, 3, 1, 2).astype(dtype)                 # [n,c,y,x]
    Cm, Sm = twiddles(N, dtype)
    yc, ys = a @ Cm, a @ Sm                                                            # [n,c,y,v]
    return Cm @ yc - Sm @ ys, -(Cm @ ys + Sm @ yc)


def reduce_rings(P, N):
    table, counts = rings(N)
    out = np.zeros(P.shape[:2] + (len(counts),), np.float64)
    for b in range(len(counts)):
        out[..., b] = P[..., table == b].astype(np.float64).sum(axis=-1) / counts[b]
    return out


def spectrum(x):
    """uint8 [n,N,N,c] -> float64 [n,c,B]: the mean over each ring of |F|^2 / N^2."""
    re, im = transform(x)
    return reduce_rings((re ** 2 + im ** 2) / x.shape[1] ** 2, x.shape[1])


def spectrum_f32(x):
    """The kernel's arithmetic restated: fp32 twiddles and products, |F|^2 and the rings in float64, the result rounded to fp32."""
    re, im = transform(x, np.float32)
    P = re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2
    return (reduce_rings(P, x.shape[1]) / x.shape[1] ** 2).astype(np.float32)


def bound(x):
    """The header's bound on |out - exact| per image, channel and ring, float64 [n,c,B]:
    delta = g sum |a|, g = sqrt(2) (2N + 8) u / (1 - (2N + 8) u); E = (2 mean_ring|F| delta + delta^2) / N^2;
    E + 2 u (exact + E) + 2^-149."""
    x = np.asarray(x)
    N = x.shape[1]
    g = np.sqrt(2.0) * (2 * N + 8) * U / (1.0 - (2 * N + 8) * U)
    delta = g * np.abs(x.astype(np.float64) - 128).sum(axis=(1, 2))                     # [n,c]
    re, im = transform(x)
    mean_abs = reduce_rings(np.sqrt(re ** 2 + im ** 2), N)
    exact = reduce_rings((re ** 2 + im ** 2) / N ** 2, N)
    E = (2.0 * mean_abs * delta[..., None] + delta[..., None] ** 2) / N ** 2
    return E + 2.0 * U * (exact + E) + 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------------ the numbers
def compare(g, r, N):
    """Segment means g, r [c,B] -> the four numbers, nan where undefined."""
    _, counts = rings(N)
    c, B = g.shape
    nan = float("nan")
    D = np.full((c, B), np.nan)
    for ch in range(c):
        for b in range(B):
            if g[ch, b] > 0 and r[ch, b] > 0:
                D[ch, b] = 10.0 * np.log10(g[ch, b] / r[ch, b])
    sq = [D[ch, b] ** 2 for ch in range(c) for b in range(1, B) if not np.isnan(D[ch, b])]
    out = dict(spectral_distance=float(np.sqrt(np.mean(sq))) if sq else nan)
    hf = []
    for s in (g, r):
        top = sum(counts[b] * s[ch, b] for ch in range(c) for b in range(1, B) if 4 * b > N)
        all_ = sum(counts[b] * s[ch, b] for ch in range(c) for b in range(1, B))
        hf.append(top / all_ if all_ > 0 else 0.0)
    out["high_frequency_db"] = float(10.0 * np.log10(hf[0] / hf[1])) if hf[0] > 0 and hf[1] > 0 else nan
    for name, b in (("nyquist_db", N // 2), ("checkerboard_db", B - 1)):
        v = [D[ch, b] for ch in range(c) if not np.isnan(D[ch, b])]
        out[name] = float(np.mean(v)) if N % 2 == 0 and v else nan
    return out


NAMES = ("spectral_distance", "high_frequency_db", "nyquist_db", "checkerboard_db")


def _nanmean(v):
    v = [e for e in v if not np.isnan(e)]
    return float(np.mean(v)) if v else float("nan")


def evaluate(real, real_labels, gen, labels, K, spectrum_fn=spectrum):
    """The evaluator's result from the definition; ``spectrum_fn`` gives the per-image spectra (float64 here, fp32-restated for the
    tolerance measurement)."""
    real_labels, labels = np.asarray(real_labels).reshape(-1), np.asarray(labels).reshape(-1)
    rk, gk = (real_labels >= 0) & (real_labels < K), (labels >= 0) & (labels < K)
    N = real.shape[1]
    Sr, Sg = np.asarray(spectrum_fn(real[rk]), np.float64), np.asarray(spectrum_fn(gen[gk]), np.float64)
    yr, yg = real_labels[rk], labels[gk]
    out = compare(Sg.mean(axis=0), Sr.mean(axis=0), N)
    per = {name: np.full(K, np.nan) for name in NAMES}
    floor_per = np.full(K, np.nan)
    left, undefined = [], []
    for k in range(K):
        g, r = Sg[yg == k], Sr[yr == k]
        if min(len(g), len(r)) < 2:
            left.append(k)
        else:
            res = compare(g.mean(axis=0), r.mean(axis=0), N)
            if np.isnan(res["spectral_distance"]):
                undefined.append(k)
            else:
                for name in NAMES:
                    per[name][k] = res[name]
        m = min(len(g), len(r) // 2)
        if m >= 2:
            floor_per[k] = compare(r[:m].mean(axis=0), r[m:2 * m].mean(axis=0), N)["spectral_distance"]
    for name in NAMES:
        out["per_class_" + name] = per[name]
        out["intra_class_" + name] = _nanmean(per[name])
    d = [v for v in per["spectral_distance"] if not np.isnan(v)]
    out["intra_class_spectral_distance_se"] = float(np.std(d, ddof=1) / np.sqrt(len(d))) if len(d) >= 2 else float("nan")
    m = min(len(Sg), len(Sr) // 2)
    out["floor_spectral_distance"] = compare(Sr[:m].mean(axis=0), Sr[m:2 * m].mean(axis=0), N)["spectral_distance"] if m >= 2 else float("nan")
    out["floor_per_class_spectral_distance"] = floor_per
    out["floor_intra_class_spectral_distance"] = _nanmean(floor_per)
    out.update(classes_used=len(d), left_out=left, undefined=undefined, rejected_real=int((~rk).sum()), rejected_generated=int((~gk).sum()))
    return out


def relative_difference(a, b):
    """The largest relative difference between two results over every float key (arrays entry by entry; nan must meet nan)."""
    worst = 0.0
    for key, va in a.items():
        if key in ("classes_used", "left_out", "undefined", "rejected_real", "rejected_generated"):
            assert va == b[key], key
            continue
        va, vb = np.atleast_1d(np.asarray(va, np.float64)), np.atleast_1d(np.asarray(b[key], np.float64))
        assert np.array_equal(np.isnan(va), np.isnan(vb)), key
        ok = ~np.isnan(va)
        if ok.any():
            worst = max(worst, float((np.abs(va[ok] - vb[ok]) / np.maximum(np.abs(va[ok]), 1e-300)).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ images
def blurred_noise(rs, n, N, c, taps=3, sigma=40.0):
    """Noise of deviation ``sigma`` around 128, smoothed by a ``taps`` x ``taps`` circular average: energy falling with frequency."""
    z = rs.randn(n, N, N, c) * sigma
    k = np.zeros(N)
    k[np.arange(taps) - taps // 2] = 1.0 / taps
    for axis in (1, 2):
        z = np.real(np.fft.ifft(np.fft.fft(z, axis=axis) * np.fft.fft(k).reshape([-1 if a == axis else 1 for a in range(4)]), axis=axis))
    return z * taps + 128.0


def quantise(z):
    return np.clip(np.rint(z), 0, 255).astype(np.uint8)


def blur3(x):
    """A 3-tap circular average along both axes of uint8 images."""
    z = x.astype(np.float64)
    for axis in (1, 2):
        z = (np.roll(z, 1, axis) + z + np.roll(z, -1, axis)) / 3.0
    return quantise(z)


def checkerboard(N, amplitude):
    y, x = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return amplitude * (1 - 2 * ((y + x) % 2)).astype(np.float64)[None, :, :, None]


def stripes(N, amplitude):
    return amplitude * (1 - 2 * (np.arange(N) % 2)).astype(np.float64)[None, None, :, None] * np.ones((1, N, 1, 1))


def families(N, c, n, seed=0):
    """name -> uint8 [n,N,N,c]: the kernel test's image families."""
    rs = np.random.RandomState(seed + 1000 * N + c)
    out = dict(uniform=rs.randint(0, 256, size=(n, N, N, c)).astype(np.uint8))
    for v in (0, 128, 255):
        out["constant_%d" % v] = np.full((n, N, N, c), v, np.uint8)
    out["checkerboard"] = quantise(127.5 + np.broadcast_to(checkerboard(N, 127.5), (n, N, N, c)))
    out["stripes"] = quantise(127.5 + np.broadcast_to(stripes(N, 127.5), (n, N, N, c)))
    imp = np.full((n, N, N, c), 128, np.uint8)
    for i in range(n):
        imp[i, (3 * i + 1) % N, (5 * i + 2) % N, :] = (37 * i + 200) % 256
    out["impulse"] = imp
    k = 1 + np.arange(n) % (N // 2)
    out["cosine"] = quantise(128 + 100 * np.cos(2 * np.pi * k[:, None, None, None] * np.arange(N)[None, None, :, None] / N) * np.ones((1, N, 1, c)))
    out["blurred_noise"] = quantise(blurred_noise(rs, n, N, c))
    names = sorted(out)
    out["mixed"] = np.stack([out[names[i % len(names)]][i] for i in range(n)])
    return out


def world(K, per_class, N, c, seed=0):
    """The image sets of the ordering and end-to-end tests: a real set of 2 per_class images per class (every class its own
    brightness and smoothing), a fresh draw of per_class per class, that draw blurred, with a +-6 checkerboard, with +-6 stripes."""
    rs = np.random.RandomState(seed)
    def draw(labels):
        x = np.empty((len(labels), N, N, c))
        for k in range(K):
            rows = np.flatnonzero(labels == k)
            x[rows] = blurred_noise(rs, len(rows), N, c, taps=3, sigma=20.0 + 5.0 * k) + 6.0 * (k - K / 2.0)
        return x
    real_labels = np.random.RandomState(seed + 1).permutation(np.repeat(np.arange(K), 2 * per_class))
    labels = np.random.RandomState(seed + 2).permutation(np.repeat(np.arange(K), per_class))
    real, fresh = draw(real_labels), draw(labels)
    return dict(real=quantise(real), real_labels=real_labels, labels=labels, fresh=quantise(fresh), blurred=blur3(quantise(fresh)),
                checker=quantise(fresh + checkerboard(N, 6.0)), striped=quantise(fresh + stripes(N, 6.0)))


def orderings(floor, fresh, blurred, checker, striped):
    """The orderings of the issue's table on results with the evaluator's keys (``floor``: a distance)."""
    assert fresh["spectral_distance"] < 3.0 * floor                                  # the same distribution scores like the floor
    assert blurred["spectral_distance"] > 5.0 * fresh["spectral_distance"] and blurred["high_frequency_db"] < -2.0
    assert abs(fresh["high_frequency_db"]) < 0.5
    assert checker["checkerboard_db"] > 5.0 and abs(checker["nyquist_db"]) < 1.0 and abs(fresh["checkerboard_db"]) < 2.0
    assert checker["spectral_distance"] > fresh["spectral_distance"]
    assert striped["nyquist_db"] > 2.0 and abs(striped["checkerboard_db"]) < 2.0 and abs(fresh["nyquist_db"]) < 1.0
