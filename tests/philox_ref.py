"""The device random stream restated in numpy for the tests: Philox4x32-10 over a general 4-word counter and 2-word key (checked
against the published Random123 vectors in test_philox_ref_cpu.py), and on top of it the stream of csrc/rng.h as include/rcgan_hip.h
describes it (rcgan_rng_fill).  The product never imports this module.

  quad q of a stream = philox((lo32(offset + q), hi32(offset + q), 0x5eed5eed, 0), (lo32(seed), hi32(seed)))
  uniform            = lo + (hi - lo) * ((r >> 8) * 2^-24) in float32, kept below hi
  normal             = Box-Muller on the lane pairs (0, 1) and (2, 3), u = ((float)(r >> 8) + 0.5f) * 2^-24 in float32
"""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_C2 = 0x5EED5EED
TWO_PI_F32 = np.float32(6.28318530718)
INV24 = np.float32(2.0 ** -24)

# Where the stream of seed 1234 holds an extreme 24-bit word (r >> 8), as (quad, lane): found by a search of quads 0 .. 2^24,
# re-derived in test_philox_ref_cpu.py.  The range tests of rcgan_rng_fill start a draw of 4 at these quads.
EXTREME_SEED = 1234
ALL_ONES_WORDS = ((595913, 1), (4657129, 3), (6646469, 3), (9807947, 1), (12657600, 1))
ZERO_WORDS = ((5347049, 1), (5350946, 0), (11589248, 1))
ALL_ONES_EVEN_LANE = (23049296, 0)      # the first all-ones word in a lane that feeds u1 of the normal transform (search went on to 2^25)


def philox4x32(counter, key, rounds=10):
    """counter [..., 4], key [..., 2] (anything uint32-valued, broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, np.uint64) & MASK
    k = np.asarray(key, np.uint64) & MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0           # 32 x 32 -> 64 bit: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def stream_quads(seed, first_quad, nquads):
    """Quads first_quad .. first_quad + nquads - 1 of the stream of ``seed`` (both 64-bit, the offset wraps) -> [nquads, 4] uint32."""
    ctr = [(int(first_quad) + q) & 0xFFFFFFFFFFFFFFFF for q in range(int(nquads))]
    c = np.empty((len(ctr), 4), np.uint64)
    c[:, 0] = [v & 0xFFFFFFFF for v in ctr]
    c[:, 1] = [v >> 32 for v in ctr]
    c[:, 2] = STREAM_C2
    c[:, 3] = 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32(c, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def stream_words(seed, first_quad, count):
    """The ``count`` words a draw of ``count`` numbers starting at quad ``first_quad`` consumes (its last quad may be cut)."""
    return stream_quads(seed, first_quad, (int(count) + 3) // 4).reshape(-1)[:int(count)]


def quads_of(count):
    """What a draw of ``count`` numbers advances the stream by."""
    return (int(count) + 3) // 4


def unit24(words):
    """(r >> 8) * 2^-24: exact in float32."""
    return (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * INV24


def below(x):
    """The largest float32 below x."""
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def _fma_f32(a, b, c):
    """round_float32(a * b + c) with ONE rounding (exact rational arithmetic)."""
    out = np.empty(len(b), np.float32)
    fa, fc = Fraction(float(a)), Fraction(float(c))
    for i, v in enumerate(b):
        exact = fa * Fraction(float(v)) + fc
        f = np.float32(float(exact))                  # float(Fraction) rounds once to float64; repair the second rounding below
        if Fraction(float(f)) != exact:
            lo_n, hi_n = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
            best = min((lo_n, f, hi_n), key=lambda t: (abs(Fraction(float(t)) - exact), int(np.float32(t).view(np.uint32)) & 1))
            f = np.float32(best)
        out[i] = f
    return out


def uniform(words, lo, hi):
    """-> (unfused, fused): float32 lo + (hi - lo) * u with the product rounded, and with one rounding for product and sum (the
    compiler may contract them into a fused multiply-add); both kept below hi.  For lo = 0 the two are the same number hi * u."""
    lo, hi = np.float32(lo), np.float32(hi)
    u = unit24(words)
    d = np.float32(hi - lo)
    cap = below(hi)
    unfused = np.minimum((lo + (d * u).astype(np.float32)).astype(np.float32), cap)
    fused = unfused if lo == 0 else np.minimum(_fma_f32(d, u, lo), cap)
    return unfused, fused


def normal_u(words):
    """((float)(r >> 8) + 0.5f) * 2^-24 in float32: the + 0.5f rounds to even from r >> 8 = 2^23 on, 0xFFFFFF gives 1.0."""
    r = (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32)
    return ((r + np.float32(0.5)).astype(np.float32) * INV24).astype(np.float32)


def normal(words, mean, std):
    """Box-Muller on the lane pairs of whole quads (len(words) a multiple of 4, or cut after the draw: pass the quads and slice) ->
    float64.  u1, u2 and the angle 6.28318530718f * u2 are the float32 values the kernel forms; log / sqrt / cos / sin are float64."""
    w = np.asarray(words, np.uint32).reshape(-1, 2)
    u1 = normal_u(w[:, 0]).astype(np.float64)
    ang = (TWO_PI_F32 * normal_u(w[:, 1])).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    out = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)
    return float(np.float32(mean)) + float(np.float32(std)) * out


def normal_bound(ref, std):
    """|got - ref| allowed for a float32 Box-Muller value: 8e-6 * std + one float32 ulp of |ref|.  The float32 rounding of the angle
    is at most 2^-24 * 2 pi = 3.7e-7 rad and the radius at most sqrt(-2 ln(0.5 * 2^-24)) = 5.887, together 2.2e-6; the rest leaves a
    few ulp each to logf, sqrtf, cosf and sinf."""
    return 8e-6 * abs(float(std)) + np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


RADIUS_MAX = float(np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -24)))      # 5.887
