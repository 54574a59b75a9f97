"""The LeCam regulariser without a GPU: the ABI declares and exports its three entry points, the model and the command line refuse bad
arguments before a context exists, the float64 restatement (tests/lecam_ref.py, the reference of the GPU tests) has the gradients float64
autograd gives for the same cost, and the update sequence has the properties the definition states."""
import os
import re

import numpy as np
import pytest
import torch

from tests import head_loss_ref as R
from tests import lecam_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rcgan_loss_reg_fwd_bwd", "rcgan_proj_head_reg_fwd_bwd", "rcgan_lecam_update")


def test_header_binding_and_both_builds_have_the_three_entry_points():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    # the plain entry points' signatures with one more pointer; the update's eleven arguments
    assert len(_lib.SIGNATURES["rcgan_loss_reg_fwd_bwd"][1]) == len(_lib.SIGNATURES["rcgan_loss_fwd_bwd"][1]) + 1
    assert len(_lib.SIGNATURES["rcgan_proj_head_reg_fwd_bwd"][1]) == len(_lib.SIGNATURES["rcgan_proj_head_fwd_bwd"][1]) + 1
    assert len(_lib.SIGNATURES["rcgan_lecam_update"][1]) == 11
    assert [f[0] for f in _lib.LossReg._fields_] == ["weight", "anchor_a", "anchor_b", "gate", "reg_acc"]
    assert "a_R, a_F, updates, mean_real_last, mean_fake_last, skipped, 0, 0" in hdr
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
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lecam must be"):
            cifar.CifarRCGAN(lecam=bad)
    for bad in (1.0, -0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lecam_decay"):
            cifar.CifarRCGAN(lecam=0.3, lecam_decay=bad)
    # the decay's range holds with the option off too
    with pytest.raises(ValueError, match="lecam_decay"):
        cifar.CifarRCGAN(lecam_decay=1.0)
    with pytest.raises(ValueError, match="world_size = 2"):
        cifar.CifarRCGAN(lecam=0.3, world_size=2, comm="stub")
    assert cifar.check_lecam(0.3, 0.99) == (0.3, 0.99)
    assert cifar.check_lecam(0, 0.0) == (0.0, 0.0)
    assert cifar.check_lecam(0.0, 0.99, world_size=8) == (0.0, 0.99)          # off: any world


def test_command_line_refuses_bad_flags_before_any_gpu_work(monkeypatch, tmp_path):
    cifar = _no_context(monkeypatch)
    from rcgan_amd import train_cifar
    base = ["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--synthetic"]
    f = train_cifar.define_flags().parse(base + ["--lecam", "0.3", "--lecam_decay", "0.9"])
    assert (f.lecam, f.lecam_decay) == (0.3, 0.9)
    d = train_cifar.define_flags().parse(base)
    assert (d.lecam, d.lecam_decay) == (0.0, 0.99)
    for extra, match in ((["--lecam", "-1"], "lecam must be"),
                         (["--lecam", "0.3", "--lecam_decay", "1.0"], "lecam_decay"),
                         (["--lecam_decay", "-0.5"], "lecam_decay")):
        with pytest.raises(ValueError, match=match):
            train_cifar.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="world_size = 2"):
        train_cifar.main(base + ["--lecam", "0.3", "--ngpus", "2"])
    assert cifar.Context is not None


# ---------------------------------------------------------------------------------------------- the term and its gradients
def _torch_term(kind, x):
    if kind == R.HINGE_REAL:
        return torch.relu(1 - x)
    if kind == R.HINGE_FAKE:
        return torch.relu(1 + x)
    if kind == R.NEG_MEAN:
        return -x
    z = 1.0 if kind == R.CE_ONES else 0.0
    return torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))


@pytest.mark.parametrize("kind", [R.HINGE_REAL, R.HINGE_FAKE, R.NEG_MEAN, R.CE_ONES, R.CE_ZEROS])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("gate", [None, 0.0, 1.0, 7.0])
def test_reference_gradients_against_float64_autograd(kind, weighted, gate):
    rs = np.random.RandomState(10 * kind + weighted)
    rows, cols, weight, lam, a, scale = 7, 5, 1.7, 0.3, 0.4, 8.0
    x = rs.randn(rows, cols) * 2
    w = rs.randn(rows, cols) if weighted else None              # (negative entries: the C^-1 rows have them)
    ref = LR.loss_reg_fwd_bwd(kind, x, w, weight, lam, a, gate, scale=scale)
    tx = torch.tensor(x, requires_grad=True)
    tw = torch.tensor(w, requires_grad=True) if weighted else None
    on = gate is None or gate > 0
    t = _torch_term(kind, tx) + (lam * (tx - a) ** 2 if on else 0.0)
    cost = weight * ((t * tw).sum(1).mean() if weighted else t.mean())
    cost.backward()
    np.testing.assert_allclose(ref["value"], float(cost.detach()), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref["dlogit"], scale * tx.grad.numpy(), rtol=1e-12, atol=1e-15)
    if weighted:
        np.testing.assert_allclose(ref["dwts"], scale * tw.grad.numpy(), rtol=1e-12, atol=1e-15)
    q = (x - a) ** 2
    want_R = ((q * w).sum(1).mean() if weighted else q.mean()) if on else 0.0
    np.testing.assert_allclose(ref["R"], want_R, rtol=1e-13, atol=1e-15)
    # lambda = 0 and a closed gate are the plain term
    plain = R.loss_fwd_bwd(kind, x, w, weight, scale)
    for off in (LR.loss_reg_fwd_bwd(kind, x, w, weight, 0.0, a, gate, scale=scale), LR.loss_reg_fwd_bwd(kind, x, w, weight, lam, a, 0.0, scale=scale)):
        assert off["value"] == plain[0] and np.array_equal(off["dlogit"], plain[2]) and np.array_equal(off["dwts"], plain[3]) and off["R"] == 0


def test_inactive_hinges_leave_exactly_the_regularisers_gradient():
    x = np.array([[1.5], [2.0], [7.0]])
    ref = LR.loss_reg_fwd_bwd(R.HINGE_REAL, x, None, 1.0, 0.25, -0.5, 1.0)
    np.testing.assert_allclose(ref["dlogit"], 2 * 0.25 * (x + 0.5) / 3, rtol=1e-15)       # (the loss part: exactly zero)
    np.testing.assert_allclose(ref["value"], 0.25 * ((x + 0.5) ** 2).mean(), rtol=1e-15)
    assert not R.loss_fwd_bwd(R.HINGE_REAL, x, None, 1.0)[2].any()


# ---------------------------------------------------------------------------------------------- the scores and the update
def test_scores():
    lg = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    assert LR.scores(lg[:, :1])[0].tolist() == [1, 5, 9]
    assert LR.scores(lg, labels=[3, 0, 2])[0].tolist() == [4, 5, 11]
    assert LR.scores(lg, labels=[4, -1, 2])[0].tolist() == [0, 0, 11]          # a label outside the row counts as zero ...
    assert LR.batch_mean(lg, labels=[4, -1, 2])[0] == 11 / 3                   # ... and stays in the denominator
    w = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [2, 0, 0, -1]], np.float64)  # rows that sum to 1, one with a negative entry
    assert LR.scores(lg, wts=w)[0].tolist() == [1, 5.5, 18 - 12]
    assert LR.batch_mean(lg, wts=w)[2] == 12


def test_first_update_sets_the_anchors_then_the_average_moves():
    s = LR.update(LR.new_state(), 2.0, -3.0, 0.9)
    assert s.tolist() == [2.0, -3.0, 1.0, 2.0, -3.0, 0.0, 0.0, 0.0]
    s = LR.update(s, 4.0, 1.0, 0.9)
    np.testing.assert_allclose(s[:5], [0.9 * 2 + 0.1 * 4, 0.9 * -3 + 0.1 * 1, 2, 4, 1], rtol=1e-15)
    # a constant batch mean is a fixed point
    t = LR.update(LR.new_state(), 1.5, -1.5, 0.99)
    for _ in range(20):
        t = LR.update(t, 1.5, -1.5, 0.99)
    np.testing.assert_allclose(t[:2], [1.5, -1.5], rtol=1e-14)
    assert t[LR.UPDATES] == 21 and t[LR.SKIPPED] == 0


def test_decay_zero_tracks_the_batch():
    s = LR.new_state()
    for k in range(1, 6):
        s = LR.update(s, float(k), -float(k), 0.0)
        assert s[LR.A_REAL] == k and s[LR.A_FAKE] == -k and s[LR.UPDATES] == k


def test_a_non_finite_mean_is_skipped_and_leaves_everything_else_alone():
    s = LR.update(LR.new_state(), 2.0, -3.0, 0.9)
    for bad in ((np.inf, 0.0), (0.0, -np.inf), (np.nan, 0.0), (1.0, np.nan)):
        t = LR.update(s, bad[0], bad[1], 0.9)
        assert np.array_equal(np.delete(t, LR.SKIPPED), np.delete(s, LR.SKIPPED)) and t[LR.SKIPPED] == s[LR.SKIPPED] + 1
        s = t
    assert s[LR.SKIPPED] == 4 and s[LR.UPDATES] == 1
    # before the first update too: the gate stays closed
    t = LR.update(LR.new_state(), np.nan, 1.0, 0.9)
    assert t[LR.UPDATES] == 0 and t[LR.SKIPPED] == 1 and not t[:2].any()
    # an inf logit in the batch makes the mean non-finite
    lg = np.array([[1.0], [np.inf], [2.0], [3.0]], np.float32)
    t, _ = LR.update_from_logits(LR.new_state(), lg, 2, 0.9)
    assert t[LR.SKIPPED] == 1 and t[LR.UPDATES] == 0
