"""The diversity-sensitive generator term without a GPU: the ABI declares and exports its entry point, the float64 restatement
(tests/diversity_ref.py, the reference of the GPU tests) has the gradient float64 autograd gives for the same expression, the masking
rules and the -1 sentinel, the model and the command line refuse bad arguments before a context exists, and the label pairing helper
has the properties the engine relies on."""
import os
import re

import numpy as np
import pytest
import torch

from tests import diversity_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rcgan_pair_diversity_workspace_bytes", "rcgan_pair_diversity_fwd_bwd")


def test_header_binding_and_both_builds_have_the_entry_point():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["rcgan_pair_diversity_fwd_bwd"][1]) == 16
    for lib in (_lib.load(), _lib.load("f16")):
        for name in NAMES:
            assert hasattr(lib, name), name
        assert lib.rcgan_pair_diversity_workspace_bytes(64) == 256 and lib.rcgan_pair_diversity_workspace_bytes(0) == 0
    assert callable(ops.pair_diversity)
    assert "diversity.hip" in open(os.path.join(ROOT, "robust-conditional-gan_amd", "csrc", "build.sh")).read()


# ---------------------------------------------------------------------------------------------- the term and its gradient
def _inputs(seed, p, d, zd):
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, (2 * p, d)), rs.randn(2 * p, zd)


@pytest.mark.parametrize("tau", [np.inf, 0.6])
@pytest.mark.parametrize("labelled", [False, True])
def test_reference_gradient_against_float64_autograd(tau, labelled):
    p, d, zd, weight, scale = 6, 37, 5, 1.7, 8.0
    x, z = _inputs(3, p, d, zd)
    x[p:p + 2] = x[:2] + 0.2 * (x[p:p + 2] - x[:2])            # two close pairs: ratios on both sides of tau = 0.6
    labels = np.array([0, 1, 2, 3, 4, 5, 0, 1, 9, 3, 4, 5]) if labelled else None          # pair 2 has unequal labels
    ref = DR.pair_diversity(x, z, labels, weight, tau, scale=scale)
    # the conditions under which autograd and the analytic gradient must agree: no zero difference, no ratio at the clamp
    assert np.all(x[:p] != x[p:])
    assert DR.min_relative_gap_to_tau(ref, tau) >= 1e-3
    if np.isfinite(tau):
        assert ref["clamped"].any() and (ref["mask"] & ~ref["clamped"]).any()
    tx = torch.tensor(x, requires_grad=True)
    tz = torch.tensor(z)
    r = (tx[:p] - tx[p:]).abs().mean(1) / (tz[:p] - tz[p:]).abs().mean(1)
    m = torch.ones(p, dtype=torch.float64)
    if labelled:
        m[2] = 0
    cost = -(weight / p) * (m * torch.clamp(r, max=tau)).sum()
    cost.backward()
    np.testing.assert_allclose(ref["loss"], float(cost.detach()), rtol=1e-13)
    np.testing.assert_allclose(ref["dx"], scale * tx.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(ref["ratio"][ref["mask"]], r.detach().numpy()[ref["mask"]], rtol=1e-13)
    # the loss value is not scaled
    assert DR.pair_diversity(x, z, labels, weight, tau, scale=1.0)["loss"] == ref["loss"]
    # weight 0: nothing
    off = DR.pair_diversity(x, z, labels, 0.0, tau)
    assert off["loss"] == 0 and not off["dx"].any()


def test_masking_rules_and_the_sentinel():
    p, d, zd = 4, 12, 3
    x, z = _inputs(5, p, d, zd)
    z[p + 1] = z[1]                                          # pair 1: identical latents
    x[p + 3] = x[3]                                          # pair 3: identical images (NOT masked: ratio 0, gradient 0)
    labels = np.array([2, 2, 2, 2, 2, 2, 7, 2])              # pair 2: unequal labels
    ref = DR.pair_diversity(x, z, labels, 1.0, np.inf)
    assert ref["mask"].tolist() == [True, False, False, True]
    assert ref["ratio"][1] == -1.0 and ref["ratio"][2] == -1.0 and ref["ratio"][0] > 0 and ref["ratio"][3] == 0.0
    assert np.isnan(ref["raw"][1]) and ref["raw"][2] > 0      # an unequal-label pair still HAS a ratio; it just does not count
    # masked pairs: no gradient on either row, and no term -- but they stay in the denominator P
    for i in (1, 2, 3):
        assert not ref["dx"][i].any() and not ref["dx"][i + p].any()
    assert ref["dx"][0].all() and np.array_equal(ref["dx"][0], -ref["dx"][p])
    assert ref["loss"] == -(ref["ratio"][0] + 0.0) / p
    # without labels pair 2 counts
    assert DR.pair_diversity(x, z, None, 1.0, np.inf)["mask"].tolist() == [True, False, True, True]
    # sgn(0) = 0: one equal element gets no gradient, its neighbours do
    x[p, 4] = x[0, 4]
    g = DR.pair_diversity(x, z, labels, 1.0, np.inf)["dx"]
    assert g[0, 4] == 0 and g[p, 4] == 0 and g[0, 3] != 0
    # the report: mean over unmasked pairs, shares of P
    rep = DR.report(ref["ratio"], np.inf)
    assert rep["masked"] == 0.5 and rep["clamped"] == 0.0 and rep["ratio_mean"] == ref["ratio"][[0, 3]].mean()
    assert DR.report(np.array([-1.0, -1.0]), 1.0) == dict(ratio_mean=None, clamped=0.0, masked=1.0)
    assert DR.report(np.array([0.5, 2.0, 1.0, -1.0]), 1.0)["clamped"] == 0.5


def test_a_pair_at_the_clamp_counts_as_clamped():
    x = np.array([[1.0, 0.0], [0.0, 0.0]])
    z = np.array([[1.0], [0.0]])
    ref = DR.pair_diversity(x, z, None, 2.0, 0.5)            # r = 0.5 exactly = tau
    assert ref["clamped"].tolist() == [True] and not ref["dx"].any() and ref["loss"] == -1.0


# ---------------------------------------------------------------------------------------------- arguments
def _no_context(monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar

    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cifar, "Context", no_context)
    return cifar


def test_check_diversity_and_the_constructor_before_a_context_exists(monkeypatch):
    cifar = _no_context(monkeypatch)
    assert cifar.check_diversity(0, float("inf")) == (0.0, float("inf"))
    assert cifar.check_diversity(1, 0.8) == (1.0, 0.8)
    assert cifar.check_diversity(0.5, float("inf")) == (0.5, float("inf"))
    assert cifar.check_diversity(0.0, 0.8, world_size=8) == (0.0, 0.8)           # off: any world
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="diversity must be"):
            cifar.check_diversity(bad, 1.0)
        with pytest.raises(ValueError, match="diversity must be"):
            cifar.CifarRCGAN(diversity=bad)
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="diversity_tau must be"):
            cifar.check_diversity(1.0, bad)
        with pytest.raises(ValueError, match="diversity_tau must be"):
            cifar.CifarRCGAN(diversity=1.0, diversity_tau=bad)
    with pytest.raises(ValueError, match="diversity_tau must be"):               # the clamp's range holds with the option off too
        cifar.CifarRCGAN(diversity_tau=0.0)
    with pytest.raises(ValueError, match="world_size = 2"):
        cifar.check_diversity(1.0, 1.0, world_size=2)
    with pytest.raises(ValueError, match="world_size = 2"):
        cifar.CifarRCGAN(diversity=1.0, world_size=2, comm="stub")


def test_pair_generator_labels():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import pair_generator_labels
    rs = np.random.RandomState(0)
    B = 8
    rnd, bia = rs.randint(10, size=2 * B).astype(np.int32), rs.randint(10, size=2 * B).astype(np.int32)
    rnd0, bia0 = rnd.copy(), bia.copy()
    r, b = pair_generator_labels(rnd, bia, B)
    assert np.array_equal(rnd, rnd0) and np.array_equal(bia, bia0)               # the inputs are left alone
    assert r.shape == (2 * B,) and b.shape == (2 * B,) and r.dtype == rnd.dtype and b.dtype == bia.dtype
    assert np.array_equal(r[:B], rnd0[:B]) and np.array_equal(r[B:], rnd0[:B])   # rows B..2B take rows 0..B
    assert np.array_equal(b, bia0)                                               # the biased labels stay as drawn
    assert not np.array_equal(rnd0[B:], rnd0[:B])                                # (the draw was not paired by chance)
    r2, _ = pair_generator_labels(r, b, B)
    assert np.array_equal(r2, r)                                                 # idempotent
    for bad in (rnd0[:-1], rnd0.reshape(2, B)):
        with pytest.raises(ValueError, match="pair_generator_labels"):
            pair_generator_labels(bad, bia0, B)


def test_command_line_parses_and_refuses_before_any_gpu_work(monkeypatch, tmp_path):
    cifar = _no_context(monkeypatch)
    from rcgan_amd import train_cifar
    base = ["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--synthetic"]
    f = train_cifar.define_flags().parse(base + ["--diversity", "1", "--diversity_tau", "0.8"])
    assert (f.diversity, f.diversity_tau) == (1.0, 0.8)
    d = train_cifar.define_flags().parse(base)
    assert (d.diversity, d.diversity_tau) == (0.0, float("inf"))
    assert train_cifar.define_flags().parse(base + ["--diversity_tau", "inf"]).diversity_tau == float("inf")
    defs = train_cifar.define_flags()._defs
    assert "not tuned" in defs["diversity"][2] and "not tuned" in defs["diversity_tau"][2]
    for extra, match in ((["--diversity", "-1"], "diversity must be"),
                         (["--diversity", "nan"], "diversity must be"),
                         (["--diversity", "1", "--diversity_tau", "0"], "diversity_tau must be"),
                         (["--diversity_tau", "-0.5"], "diversity_tau must be")):
        with pytest.raises(ValueError, match=match):
            train_cifar.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="world_size = 2"):
        train_cifar.main(base + ["--diversity", "1", "--ngpus", "2"])
    assert cifar.Context is not None
