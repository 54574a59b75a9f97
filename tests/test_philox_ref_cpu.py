"""tests/philox_ref.py against what does not depend on this project: the published Random123 known-answer vectors of philox4x32-10,
the structure of the stream as include/rcgan_hip.h and csrc/rng.h describe it, and float32 arithmetic done by hand.  The GPU tests
(test_gpu_elementwise.py) compare rcgan_rng_fill with this reference word for word."""
import numpy as np

from tests import philox_ref as P

# Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_random123_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert [int(v) for v in got] == list(want), (ctr, key, [hex(int(v)) for v in got])
    # ... and vectorised: the three at once, in another order
    got = P.philox4x32(np.array([k[0] for k in KAT[::-1]], np.uint64), np.array([k[1] for k in KAT[::-1]], np.uint64))
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT[::-1]]


def test_round_count_and_key_schedule_matter():
    ctr, key, want = KAT[2]
    assert P.philox4x32(np.array(ctr), np.array(key), rounds=9).tolist() != list(want)
    assert P.philox4x32(np.array(ctr), np.array(key[::-1])).tolist() != list(want)


def test_stream_layout():
    """Counter = (lo32, hi32 of offset + q, 0x5eed5eed, 0), key = (lo32, hi32 of the seed)."""
    seed = (1 << 63) + 1
    first = (1 << 32) - 2
    q = P.stream_quads(seed, first, 4)
    for i in range(4):
        o = first + i
        want = P.philox4x32(np.array([o & 0xffffffff, o >> 32, 0x5eed5eed, 0], np.uint64), np.array([1, 1 << 31], np.uint64))
        assert q[i].tolist() == want.tolist()
    assert q[1].tolist() != q[3].tolist()                                    # (2^32 - 1, 0) and (1, 1): the carry is a new counter
    assert P.stream_quads(seed, (1 << 32), 1).tolist() != P.stream_quads(seed, 0, 1).tolist()       # the high counter word is used
    assert P.stream_quads((1 << 32) + 5, 0, 1).tolist() != P.stream_quads(5, 0, 1).tolist()        # the high seed word is used
    # a draw takes whole quads and may cut the last one
    assert P.stream_words(seed, 7, 5).tolist() == P.stream_quads(seed, 7, 2).reshape(-1)[:5].tolist()
    assert [P.quads_of(c) for c in (0, 1, 3, 4, 5, 4099)] == [0, 1, 1, 1, 2, 1025]


def test_extreme_word_locations():
    """The committed (quad, lane) constants hold r >> 8 == 0xFFFFFF / 0 in the stream of seed 1234."""
    assert len(P.ALL_ONES_WORDS) >= 2 and len(P.ZERO_WORDS) >= 2
    assert P.ALL_ONES_EVEN_LANE[1] in (0, 2)
    for quad, lane in P.ALL_ONES_WORDS + (P.ALL_ONES_EVEN_LANE,):
        w = P.stream_quads(P.EXTREME_SEED, quad, 1)[0]
        assert int(w[lane]) >> 8 == 0xFFFFFF, (quad, lane, hex(int(w[lane])))
    for quad, lane in P.ZERO_WORDS:
        w = P.stream_quads(P.EXTREME_SEED, quad, 1)[0]
        assert int(w[lane]) >> 8 == 0, (quad, lane, hex(int(w[lane])))
    # the tests of the normal transform want a zero word in lane 0 (u1 smallest)
    assert any(lane == 0 for _, lane in P.ZERO_WORDS)


def test_uniform_transform_by_hand():
    ones, zero, mid = np.uint32(0xFFFFFF00), np.uint32(0xFF), np.uint32(0x80000000)
    w = np.array([ones, zero, mid], np.uint32)
    assert P.unit24(w).tolist() == [1.0 - 2.0 ** -24, 0.0, 0.5]
    for lo, hi in ((0.0, 1.0), (0.0, 1.0 / 128), (1.0, 2.0), (0.5, 1.5), (-3.0, 5.0)):
        for v in P.uniform(w, lo, hi):
            assert v.dtype == np.float32
            assert v[1] == np.float32(lo) and (v >= np.float32(lo)).all() and (v < np.float32(hi)).all(), (lo, hi, v)
    # the plain float32 expression reaches hi for (1, 2) and (0.5, 1.5): what "kept below hi" is there for
    u = P.unit24(w[:1])
    assert np.float32(1.0) + np.float32(1.0) * u[0] == np.float32(2.0)
    assert np.float32(0.5) + np.float32(1.0) * u[0] == np.float32(1.5)
    assert P.uniform(w[:1], 1.0, 2.0)[0][0] == np.float32(2.0) - np.float32(2.0 ** -23)
    # lo = 0: exactly hi * u, fused or not
    a, b = P.uniform(w, 0.0, 1.0 / 128)
    assert a is b and a.tolist() == [float(np.float32(1.0 / 128) * x) for x in P.unit24(w)]
    # one rounding against two: 1 + 3 * u with u = 1/3 rounded has a product that rounds before the sum
    words = np.arange(1, 4000, 7, dtype=np.uint32) << np.uint32(8)
    a, b = P.uniform(words, 0.1, 0.7)
    exact = np.float64(np.float32(0.1)) + np.float64(np.float32(np.float32(0.7) - np.float32(0.1))) * P.unit24(words).astype(np.float64)
    assert (np.abs(b.astype(np.float64) - exact) <= 0.5 * np.spacing(np.abs(b)) * (1 + 1e-9)).all()
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))).all()


def test_normal_transform_by_hand():
    # r >> 8 below 2^23: r + 0.5 is exact; from 2^23 on it rounds to even; 0xFFFFFF + 0.5 -> 2^24
    w = np.array([0, 1 << 8, ((1 << 23) + 1) << 8, ((1 << 23) + 2) << 8, 0xFFFFFF00], np.uint32)
    assert P.normal_u(w).tolist() == [2.0 ** -25, 1.5 * 2.0 ** -24, ((1 << 23) + 2) * 2.0 ** -24, ((1 << 23) + 2) * 2.0 ** -24, 1.0]
    # u1 -> 1.0: radius 0, the pair is exactly the mean
    z = P.normal(np.array([0xFFFFFF00, 0x12345678, 0xFFFFFF00, 0x9abcdef0], np.uint32), 0.25, 3.0)
    assert z.tolist() == [0.25] * 4
    # u1 smallest: the radius bound of the issue
    z = P.normal(np.array([0, 0, 0, 0x40000000], np.uint32), 0.0, 1.0)
    assert np.isfinite(z).all() and abs(np.hypot(z[0], z[1]) - P.RADIUS_MAX) < 1e-12 and abs(P.RADIUS_MAX - 5.887) < 1e-3
    # moments of a long draw (a sanity check of the pairing, not of the generator)
    z = P.normal(P.stream_quads(99, 0, 1 << 14).reshape(-1), 1.0, 2.0)
    assert abs(z.mean() - 1.0) < 0.03 and abs(z.std() - 2.0) < 0.03
    b = P.normal_bound(np.array([0.0, 1.0, -5.0]), 2.0)
    assert b.tolist() == [1.6e-5 + float(np.spacing(np.float32(0))), 1.6e-5 + 2.0 ** -23, 1.6e-5 + 2.0 ** -21]
