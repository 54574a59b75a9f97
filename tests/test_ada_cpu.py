"""The adaptive augmentation probability without a GPU: the ABI declares and exports the three entry points, the model and the
command line refuse bad arguments before a context exists, and the restatement of the definition (tests/ada_ref.py, the reference
of the GPU tests) has the properties the definition states."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ada_ref as A
from tests import diffaugment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rcgan_diffaugment_gated_fwd", "rcgan_diffaugment_sampled_bwd", "rcgan_ada_update")


def test_header_binding_and_both_builds_have_the_three_entry_points():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["rcgan_diffaugment_gated_fwd"][1]) == 13
    assert len(_lib.SIGNATURES["rcgan_diffaugment_sampled_bwd"][1]) == 10
    assert len(_lib.SIGNATURES["rcgan_ada_update"][1]) == 9
    assert "u7 is reserved" in hdr and "gate_u" in hdr
    for lib in (_lib.load(), _lib.load("f16")):
        for name in NAMES:
            assert hasattr(lib, name), name


def _no_context(monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar

    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cifar, "Context", no_context)
    return cifar


def test_constructor_refuses_bad_arguments_before_a_context_exists(monkeypatch):
    cifar = _no_context(monkeypatch)
    aug = "color,translation,cutout"
    with pytest.raises(ValueError, match="diffaugment"):
        cifar.CifarRCGAN(ada_target=0.6)
    with pytest.raises(ValueError, match="diffaugment"):
        cifar.CifarRCGAN(ada_target=0.6, diffaugment=" , ")
    for bad in (1.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ada_target"):
            cifar.CifarRCGAN(ada_target=bad, diffaugment=aug)
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ada_images"):
            cifar.CifarRCGAN(ada_target=0.6, ada_images=bad, diffaugment=aug)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="ada_interval"):
            cifar.CifarRCGAN(ada_target=0.6, ada_interval=bad, diffaugment=aug)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="ada_p_init"):
            cifar.CifarRCGAN(ada_target=0.6, ada_p_init=bad, diffaugment=aug)
    # the ranges hold with the option off too
    with pytest.raises(ValueError, match="ada_images"):
        cifar.CifarRCGAN(ada_images=0)
    with pytest.raises(ValueError, match="ranks would disagree on p"):
        cifar.CifarRCGAN(ada_target=0.6, diffaugment=aug, world_size=2, comm="stub")
    assert cifar.check_ada(0.6, 500000, 4, 0.0, aug) == (0.6, 500000.0, 4, 0.0)
    assert cifar.check_ada(-0.5, 1, 1, 1.0, "cutout") == (-0.5, 1.0, 1, 1.0)
    # off: no policy needed, any world
    assert cifar.check_ada(0.0, 500000, 4, 0.0, "", world_size=8)[0] == 0.0
    assert cifar.check_ada(0, 500000, 4, 0.0, aug, world_size=8)[0] == 0.0


def test_command_line_refuses_bad_flags_before_any_gpu_work(monkeypatch, tmp_path):
    cifar = _no_context(monkeypatch)
    from rcgan_amd import train_cifar
    base = ["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--synthetic"]
    aug = ["--diffaugment", "color,translation,cutout"]
    f = train_cifar.define_flags().parse(base + aug + ["--ada_target", "0.6", "--ada_images", "1000", "--ada_interval", "2",
                                                      "--ada_p_init", "0.25"])
    assert (f.ada_target, f.ada_images, f.ada_interval, f.ada_p_init) == (0.6, 1000.0, 2, 0.25)
    d = train_cifar.define_flags().parse(base)
    assert (d.ada_target, d.ada_images, d.ada_interval, d.ada_p_init) == (0.0, 500000, 4, 0.0)
    for extra, match in ((["--ada_target", "0.6"], "diffaugment"),
                         (aug + ["--ada_target", "1.0"], "ada_target"),
                         (aug + ["--ada_target", "0.6", "--ada_images", "0"], "ada_images"),
                         (aug + ["--ada_target", "0.6", "--ada_interval", "0"], "ada_interval"),
                         (aug + ["--ada_target", "0.6", "--ada_p_init", "2"], "ada_p_init")):
        with pytest.raises(ValueError, match=match):
            train_cifar.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="ranks would disagree on p"):
        train_cifar.main(base + aug + ["--ada_target", "0.6", "--ngpus", "2"])
    assert cifar.Context is not None


# ---------------------------------------------------------------------------------------------- the gated transform
def _xu(n=8, h=8, w=12, seed=0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randn(n, h, w, 3)), np.minimum(rs.uniform(size=(n, 8)).astype(np.float32), np.float32(R.U_MAX))


def test_p_zero_is_the_identity_and_p_one_is_plain_diffaugment():
    x, u = _xu()
    rs = np.random.RandomState(1)
    g = np.minimum(rs.uniform(size=(8, 4)).astype(np.float32), np.float32(R.U_MAX))
    g[0, :] = 0.0                                           # 0 < 0 is false: not even a zero gate passes p = 0
    g[1, :] = R.U_MAX                                       # the largest gate a draw can give passes p = 1
    for policy in R.POLICIES:
        assert torch.equal(A.diffaugment(x, u, g, 0.0, policy), x)
        assert (A.sample_policy(g, 0.0, policy) == 0).all()
        assert torch.equal(A.diffaugment(x, u, g, 1.0, policy), R.diffaugment(x, u, policy))
        assert (A.sample_policy(g, 1.0, policy) == policy).all()
        assert (A.sample_policy(g, float("nan"), policy) == 0).all()


def test_a_gate_equal_to_p_is_not_applied_and_all_eight_combinations_occur():
    p = np.float32(0.5)
    g = A.gate_rows(p)
    pol = A.sample_policy(g, p, 7)
    assert sorted(pol.tolist()) == list(range(8))
    assert (g[:, :3] == p).any(axis=1).sum() >= 3           # rows that hold a gate exactly at p
    for i in range(8):
        for t, bit in enumerate(A.GATE_BITS):
            if g[i, t] == p:
                assert not pol[i] & bit
            assert bool(pol[i] & bit) == bool(g[i, t] < p)
    # the next float32 below p is applied; the policy masks what the gates allow; column 3 gates nothing
    g2 = np.array([[np.nextafter(p, np.float32(0)), p, np.nextafter(p, np.float32(1)), 0.0]], np.float32)
    assert A.sample_policy(g2, p, 7).tolist() == [R.COLOR]
    assert A.sample_policy(g2, p, R.TRANSLATION | R.CUTOUT).tolist() == [0]
    # the comparison is in float32: a float64 p just above the gate rounds onto it
    assert A.sample_policy(np.array([[0.5, 0.5, 0.5, 0.5]], np.float32), 0.5 + 1e-12, 7).tolist() == [0]
    x, u = _xu()
    y = A.diffaugment(x, u, g, p, 7)
    for i in range(8):
        assert torch.equal(y[i], R.augment_one(x[i], u[i], int(pol[i])))
    assert A.gates(40, p).shape == (40, 4) and sorted(set(A.sample_policy(A.gates(40, p), p, 7).tolist())) == list(range(8))


# ---------------------------------------------------------------------------------------------- the controller
def test_sign_and_scores():
    v = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 3.0, -2.0], np.float32)
    assert A.sign(v).tolist() == [0, 0, 0, 1, -1, 1, -1, 1, -1]
    lg = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    assert A.scores(lg).tolist() == [1, 5, 9]
    assert A.scores(lg, [3, 0, 2]).tolist() == [4, 5, 11]
    assert A.scores(lg, [4, -1, 2]).tolist() == [0, 0, 11]          # a label outside the row counts as zero


def test_all_positive_scores_raise_p_by_n_interval_over_images_per_interval():
    n, interval, images = 64, 4, 4096.0
    lg = np.ones((n, 1), np.float32)
    s = A.new_state(0.0)
    for call in range(1, 13):
        s = A.update(s, lg, None, 0.6, images, interval)
        done = call // interval
        assert s[0] == np.float32(done * n * interval / images), (call, s)
        assert s[5] == done
        if call % interval == 0:
            assert s[1] == s[2] == s[3] == 0 and s[4] == 1.0        # the accumulators reset, r_last = 1
        else:
            assert (s[1], s[2], s[3]) == (n * (call % interval), n * (call % interval), call % interval)
    assert s[6] == s[7] == 0


def test_r_equal_to_target_leaves_p_unchanged_and_below_lowers_it():
    lg = np.array([[1.0], [1.0], [1.0], [-1.0]], np.float32)        # r = 0.5 exactly
    s = A.update(A.new_state(0.25), lg, None, 0.5, 16.0, 1)
    assert s[0] == np.float32(0.25) and s[4] == np.float32(0.5) and s[5] == 1
    s = A.update(A.new_state(0.25), lg, None, 0.75, 16.0, 1)
    assert s[0] == np.float32(0.0) and s[5] == 1                    # 0.25 - 4/16
    s = A.update(A.new_state(0.25), lg, None, 0.25, 16.0, 1)
    assert s[0] == np.float32(0.5)


def test_p_clamps_at_both_ends():
    up, down = np.ones((8, 1), np.float32), -np.ones((8, 1), np.float32)
    s = A.new_state(0.9)
    for _ in range(3):
        s = A.update(s, up, None, 0.6, 32.0, 1)
    assert s[0] == 1.0 and s[5] == 3
    for _ in range(6):
        s = A.update(s, down, None, 0.6, 32.0, 1)
    assert s[0] == 0.0 and s[5] == 9
    # one step larger than the whole range
    assert A.update(A.new_state(0.5), up, None, 0.0, 1.0, 1)[0] == 1.0
    assert A.update(A.new_state(0.5), down, None, 0.0, 1.0, 1)[0] == 0.0
