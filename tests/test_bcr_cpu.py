"""Balanced consistency regularisation without a GPU: the ABI declares, binds and exports the entry point, the float64 restatement
(tests/bcr_ref.py, the reference of the GPU tests) has the value and the gradients float64 autograd gives -- labelled and weighted
parts, negative weights, the weights' own gradient -- check_bcr and the constructor accept and refuse what the definition says before a
context exists, and the command line carries the three flags."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bcr_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rcgan_pair_consistency_fwd_bwd"


def test_header_binding_and_both_builds_have_the_entry_point():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, hdr)
    assert len(_lib.SIGNATURES[NAME][1]) == 13
    for lib in (_lib.load(), _lib.load("f16")):
        assert hasattr(lib, NAME)
    assert callable(ops.pair_consistency)


@pytest.mark.parametrize("pairs,cols,weighted", [(7, 1, False), (5, 10, True), (1, 3, True), (6, 4, False)])
def test_reference_against_float64_autograd(pairs, cols, weighted):
    rs = np.random.RandomState(100 * pairs + cols)
    lam, scale = 2.5, 8.0
    x, xa = rs.randn(pairs, cols), rs.randn(pairs, cols)
    w = None
    if weighted:          # rows that sum to 1 with negative entries, as the C^-1 rows of `unbiased` have them
        w = rs.randn(pairs, cols)
        w[:, 0] += 1.0 - w.sum(1)
        assert (w < 0).any() and np.allclose(w.sum(1), 1.0)
    ref = BR.pair_consistency(x[:, 0] if cols == 1 else x, xa[:, 0] if cols == 1 else xa, w, lam, scale)
    tx, txa = torch.tensor(x, requires_grad=True), torch.tensor(xa, requires_grad=True)
    tw = torch.tensor(w, requires_grad=True) if weighted else None
    c = ((tx - txa) ** 2 * tw).sum(1) if weighted else ((tx - txa) ** 2).sum(1)
    cost = lam * c.mean()
    cost.backward()
    np.testing.assert_allclose(ref["value"], float(cost.detach()), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(ref["term"], float(c.mean().detach()), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(ref["dx"], scale * tx.grad.numpy(), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(ref["dx_aug"], scale * txa.grad.numpy(), rtol=1e-13, atol=1e-300)
    if weighted:
        np.testing.assert_allclose(ref["dwts"], scale * tw.grad.numpy(), rtol=1e-13, atol=1e-300)
    else:
        assert ref["dwts"] is None


def test_identical_halves_and_zero_weight_give_exactly_nothing():
    x = np.random.RandomState(0).randn(5, 3)
    w = np.random.RandomState(1).randn(5, 3)
    ref = BR.pair_consistency(x, x.copy(), w, 10.0, 1024.0)
    assert ref["value"] == 0 and ref["term"] == 0 and not ref["dx"].any() and not ref["dx_aug"].any() and not ref["dwts"].any()
    off = BR.pair_consistency(x, x + 1, w, 0.0)
    assert off["value"] == 0 and off["term"] != 0 and not off["dx"].any() and not off["dwts"].any()


def test_the_scale_multiplies_the_gradients_only():
    rs = np.random.RandomState(3)
    x, xa, w = rs.randn(4, 2), rs.randn(4, 2), rs.randn(4, 2)
    a, b = BR.pair_consistency(x, xa, w, 3.0), BR.pair_consistency(x, xa, w, 3.0, 1024.0)
    assert a["value"] == b["value"] and a["term"] == b["term"]
    for k in ("dx", "dx_aug", "dwts"):
        assert np.array_equal(1024.0 * a[k], b[k]), k


def _no_context(monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar

    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cifar, "Context", no_context)
    return cifar


def test_check_bcr_accepts_and_refuses(monkeypatch):
    cifar = _no_context(monkeypatch)
    assert cifar.check_bcr(10, 10, "translation") == (10.0, 10.0, 2)
    assert cifar.check_bcr(0.0, 1.5, "color,cutout") == (0.0, 1.5, 5)
    assert cifar.check_bcr(2.0, 0.0, "translation") == (2.0, 0.0, 2)
    # both zero is off, whatever the policy and the world
    assert cifar.check_bcr(0.0, 0.0, "translation") == (0.0, 0.0, 0)
    assert cifar.check_bcr(0, 0, "") == (0.0, 0.0, 0)
    assert cifar.check_bcr(0.0, 0.0, "translation", world_size=8) == (0.0, 0.0, 0)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="bcr_real must be"):
            cifar.check_bcr(bad, 1.0, "translation")
        with pytest.raises(ValueError, match="bcr_fake must be"):
            cifar.check_bcr(1.0, bad, "translation")
        with pytest.raises(ValueError, match="bcr_real must be"):
            cifar.CifarRCGAN(bcr_real=bad)
    with pytest.raises(ValueError, match="non-empty bcr_policy"):
        cifar.check_bcr(1.0, 0.0, "")
    with pytest.raises(ValueError, match="non-empty bcr_policy"):
        cifar.CifarRCGAN(bcr_fake=1.0, bcr_policy=" , ")
    with pytest.raises(ValueError, match="Unknown diffaugment policy"):
        cifar.check_bcr(0.0, 0.0, "flip")          # a bad name is refused with the option off too
    with pytest.raises(ValueError, match="world_size = 2"):
        cifar.check_bcr(10, 10, "translation", world_size=2)
    with pytest.raises(ValueError, match="world_size = 2"):
        cifar.CifarRCGAN(bcr_real=10, bcr_fake=10, world_size=2, comm="stub")


def test_command_line_carries_the_flags_and_refuses_before_any_gpu_work(monkeypatch, tmp_path):
    cifar = _no_context(monkeypatch)
    from rcgan_amd import train_cifar
    base = ["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--synthetic"]
    d = train_cifar.define_flags().parse(base)
    assert (d.bcr_real, d.bcr_fake, d.bcr_policy) == (0.0, 0.0, "translation")
    f = train_cifar.define_flags().parse(base + ["--bcr_real", "10", "--bcr_fake", "5", "--bcr_policy", "translation,cutout"])
    assert (f.bcr_real, f.bcr_fake, f.bcr_policy) == (10.0, 5.0, "translation,cutout")
    for extra, match in ((["--bcr_real", "-1"], "bcr_real must be"),
                         (["--bcr_fake", "nan"], "bcr_fake must be"),
                         (["--bcr_real", "10", "--bcr_policy", ""], "non-empty bcr_policy"),
                         (["--bcr_fake", "10", "--bcr_policy", "flip"], "Unknown diffaugment policy")):
        with pytest.raises(ValueError, match=match):
            train_cifar.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="world_size = 2"):
        train_cifar.main(base + ["--bcr_real", "10", "--bcr_fake", "10", "--ngpus", "2"])
    assert cifar.Context is not None
