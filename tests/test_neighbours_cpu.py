"""Nearest-training-image metrics without a GPU: the brute-force restatement (tests/neighbours_ref.py) against a triple loop of Python
integers, the Mann-Whitney z against a hand-worked tied example, the host arithmetic of neighbours.py, the training flags, and the
argument checks of the entry point of csrc/nn_u8.hip (made before anything touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import neighbours_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nb():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import neighbours
    return neighbours


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("exclude", [False, True])
def test_the_restatement_equals_a_triple_loop_on_tiny_inputs(exclude):
    rs = np.random.RandomState(1)
    q, r = rs.randint(0, 256, size=(9, 16), dtype=np.uint8), rs.randint(0, 256, size=(11, 16), dtype=np.uint8)
    q[2] = r[7]
    r[3] = r[9] = q[5]                                                # a tie: index 3
    fill = np.uint64(12345)
    for q_off, r_off in (([0, 9], [0, 11]), ([1, 4, 4, 9, 50], [0, 5, 8, 8, 11]), ([0, 6, 2], [-3, 11, 4]), ([0, 1, 9], [0, 1, 11])):
        want = NR.best_triple_loop(q, r, q_off, r_off, exclude, fill)
        got = NR.best(q, r, q_off, r_off, exclude, fill)
        assert got.dtype == np.uint64 and (got == want).all(), (q_off, r_off)
    pooled = NR.best(q, r)
    assert pooled[2] == np.uint64(7) and pooled[5] == np.uint64(3)
    same = NR.best(r, r, [0, 1, 11], [0, 1, 11], True)
    assert same[0] == NR.ALL_ONES and same[3] == np.uint64(9) and same[9] == np.uint64(3)
    # the extremes: the largest distance a row of 12288 pixels can have
    assert NR.best(np.zeros((1, 12288), np.uint8), np.full((1, 12288), 255, np.uint8))[0] == np.uint64(799027200 << 32)
    # labelled form: rows with a foreign label drop out on either side, indices are the caller's
    d, j = NR.nearest(q, [0, 1, 0, 1, 7, 0, 1, 0, -1], r, [1, 0, 1, 0, 0, 1, 0, 0, 5, 1, 0], 2, True, False)
    assert (d[[4, 8]] == -1).all() and (j[[4, 8]] == -1).all() and j[2] == 7 and j[5] == 3
    assert all(j[k] >= 0 and [1, 0, 1, 0, 0, 1, 0, 0, 5, 1, 0][j[k]] == [0, 1, 0, 1, 7, 0, 1, 0, -1][k] for k in (0, 1, 2, 3, 5, 6, 7))


def test_the_mann_whitney_z_of_a_hand_worked_tied_example():
    nb = _nb()
    # x = 1, 2, 2 against y = 2, 3: ranks 1 | 3, 3, 3 | 5, so R_x = 7, U = 7 - 6 = 1; one tie group of 3: var = 6 / 12 (6 - 24 / 20) = 2.4
    want = (1.0 - 3.0) / np.sqrt(2.4)
    for f in (NR.mann_whitney_z, nb.mann_whitney_z):
        assert f([1, 2, 2], [2, 3]) == pytest.approx(want, rel=1e-15)
        assert f([2, 3], [1, 2, 2]) == pytest.approx(-want, rel=1e-15)
        assert f([1, 2, 3], [4, 5, 6, 7]) == pytest.approx((0.0 - 6.0) / np.sqrt(12 / 12.0 * 8), rel=1e-15)        # no ties: var = n m (N + 1) / 12
        assert np.isnan(f([], [1, 2])) and np.isnan(f([1], [])) and np.isnan(f([4, 4], [4, 4, 4]))
    rs = np.random.RandomState(2)
    x, y = rs.randint(0, 40, size=300), rs.randint(3, 50, size=200)
    assert nb.mann_whitney_z(x, y) == pytest.approx(NR.mann_whitney_z(x, y), rel=1e-12)


# --------------------------------------------------------------------------------------------------------- the host arithmetic
def test_keys_are_decoded_and_the_shares_count_only_defined_rows():
    nb = _nb()
    keys = np.array([(5 << 32) | 3, 0xFFFFFFFFFFFFFFFF, 0, (799027200 << 32) | 0xFFFFFFFE], np.uint64)
    d, j = nb.decode(keys.view(np.int64))
    assert d.tolist() == [5, -1, 0, 799027200] and j.tolist() == [3, -1, 0, 0xFFFFFFFE] and d.dtype == j.dtype == np.int64
    rho = np.array([10, -1, 4, 0])
    share, n = nb.copy_share([9, 3, 4, 0, 7], [0, 1, 2, 3, -1], rho)          # 9 < 10; rho undefined; 4 < 4 no; 0 < 0 no; no neighbour
    assert (share, n) == (1 / 3.0, 3)
    assert np.isnan(nb.copy_share([1], [-1], rho)[0]) and np.isnan(nb.copy_share([], [], rho)[0])
    assert nb.loo_accuracy([1, 5, 3, -1, 2], [2, 5, 1, 4, -1]) == (1 + 0.5 + 0 + 0 + 1) / 5.0
    assert np.isnan(nb.loo_accuracy([], []))


def test_images_are_flattened_in_one_order_and_rows_that_are_no_multiple_of_16_bytes_are_refused():
    nb = _nb()
    rows = (np.arange(2 * 3072).reshape(2, 3072) % 251).astype(np.uint8)
    x = nb.as_rows(rows)
    assert x.dtype == np.uint8 and x.shape == (2, 3072)
    assert np.array_equal(x, nb.as_rows(rows.reshape(2, 3, 32, 32).transpose(0, 2, 3, 1)))       # CHW rows and NHWC: the same pixel order
    assert nb.as_rows(np.zeros((3, 784))).shape == (3, 784) and nb.as_rows(np.zeros((3, 16, 16, 1))).shape == (3, 256)
    with pytest.raises(ValueError, match="neighbours"):
        nb.as_rows(np.zeros((2, 17, 23, 3)))
    with pytest.raises(ValueError, match="NeighbourEvaluator"):
        nb.NeighbourEvaluator(0)                                      # (checked before a context is built)


# ------------------------------------------------------------------------------------------------------------------ the flags
def test_training_flags_default_to_off_and_bad_values_are_refused_before_anything_runs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    FLAGS = train_cifar.define_flags().parse([])
    assert (FLAGS.neighbours_freq, FLAGS.neighbours_samples, FLAGS.neighbours_real_samples) == (0, 10000, 0)
    log = os.path.join(str(tmp_path), "log.txt")
    for bad in (["--neighbours_freq", "2", "--neighbours_samples", "50"], ["--neighbours_freq", "-1"], ["--neighbours_real_samples", "-1"]):
        with pytest.raises(ValueError, match="neighbours"):
            train_cifar.main(["--log_file", log] + bad)
        assert not os.path.exists(log)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_entry_point_and_check_arguments_without_a_device():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    assert re.search(r"\brcgan_nn_u8\s*\(", hdr) and "rcgan_nn_u8" in _lib.SIGNATURES
    assert hdr.index("rcgan_msssim_pairs(") < hdr.index("rcgan_nn_u8(")
    raw = (C.c_uint8 * (2 * 4 * 64 + 64))()
    base = C.addressof(raw)
    base += (-base) % 16                                              # a 16-byte aligned start inside the buffer
    qa, ra = base, base + 4 * 64
    off = (C.c_int32 * 2)(0, 4)
    best = (C.c_uint64 * 5)(*([7] * 5))
    p = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else C.cast(a, C.c_void_p))
    for lib in (_lib.load(), _lib.load("f16")):
        call = lambda nq=4, nr=4, d=64, n_seg=1, q=qa, qo=off, r=ra, ro=off, b=best: lib.rcgan_nn_u8(None, nq, nr, d, n_seg, p(q), p(qo), p(r), p(ro), 0, p(b))
        for bad in (dict(d=0), dict(d=8), dict(d=24), dict(d=12304), dict(d=-16), dict(q=qa + 4), dict(q=qa + 8), dict(r=ra + 1), dict(r=ra + 8),
                    dict(b=C.addressof(best) + 4), dict(n_seg=0), dict(n_seg=1025), dict(nq=0), dict(nr=0), dict(nq=-3),
                    dict(q=None), dict(qo=None), dict(r=None), dict(ro=None), dict(b=None)):
            assert call(**bad) == _lib.EINVALID_ARG, bad
        assert call() == _lib.EINVALID_ARG                           # legal arguments, but no context
        assert call(d=16) == _lib.EINVALID_ARG and call(d=12288) == _lib.EINVALID_ARG
        assert all(v == 7 for v in best)                             # nothing was written
