"""DiffAugment without a GPU: the ABI declares the entry points, the model refuses a bad policy before it creates a context, and the
torch restatement of the definition (tests/diffaugment_ref.py, the reference of the GPU tests) has the properties the definition
states."""
import os
import re

import numpy as np
import pytest
import torch

from tests import diffaugment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_both_entry_points():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    for name in ("rcgan_diffaugment_fwd", "rcgan_diffaugment_bwd"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    for macro, value in (("RCGAN_AUG_COLOR", 1), ("RCGAN_AUG_TRANSLATION", 2), ("RCGAN_AUG_CUTOUT", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.AUG_COLOR, _lib.AUG_TRANSLATION, _lib.AUG_CUTOUT) == (R.COLOR, R.TRANSLATION, R.CUTOUT) == (1, 2, 4)
    assert _lib.AUG_POLICIES == {"color": 1, "translation": 2, "cutout": 4}
    # both builds export them
    for lib in (_lib.load(), _lib.load("f16")):
        assert hasattr(lib, "rcgan_diffaugment_fwd") and hasattr(lib, "rcgan_diffaugment_bwd")


def test_bad_policy_is_refused_before_a_context_exists(monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar

    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cifar, "Context", no_context)
    with pytest.raises(ValueError, match="color,translation,cutout"):
        cifar.CifarRCGAN(diffaugment="colour")
    with pytest.raises(ValueError, match="color,translation,cutout"):
        cifar.CifarRCGAN(diffaugment="color,blur")
    assert cifar.parse_diffaugment("") == 0 and cifar.parse_diffaugment(None) == 0
    assert cifar.parse_diffaugment("cutout, color") == 5
    assert cifar.parse_diffaugment("color,translation,cutout") == 7


def test_policy_zero_is_the_identity():
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randn(3, 8, 12, 3))
    u = rs.uniform(size=(3, 8)).astype(np.float32)
    assert torch.equal(R.diffaugment(x, u, 0), x)


@pytest.mark.parametrize("h,w", [(32, 32), (8, 12), (4, 4)])
def test_cutout_zeroes_a_half_by_half_window_for_interior_offsets(h, w):
    x = torch.ones(1, h, w, 3, dtype=torch.float64)
    n = 0
    for oy in range(h // 4, h - h // 4 + 1):
        for ox in range(w // 4, w - w // 4 + 1):
            u = np.full((1, 8), 0.5, np.float32)
            u[0, 5], u[0, 6] = (oy + 0.5) / (h + 1), (ox + 0.5) / (w + 1)
            p = R.params(u[0], h, w, R.CUTOUT)
            assert (p["oy"], p["ox"]) == (oy, ox)
            y = R.diffaugment(x, u, R.CUTOUT)
            zero = (y == 0).all(dim=-1)
            assert int(zero.sum()) == (h // 2) * (w // 2), (oy, ox)
            assert bool(((y == 0) | (y == 1)).all())
            n += 1
    assert n >= 1
    # at the border the window is clipped: a corner offset leaves a quarter of it
    u = np.zeros((1, 8), np.float32)
    assert int((R.diffaugment(x, u, R.CUTOUT) == 0).all(dim=-1).sum()) == (h // 4) * (w // 4)


@pytest.mark.parametrize("h,w,sh,sw", [(32, 32, 4, 4), (8, 12, 1, 2), (4, 4, 1, 1)])
def test_parameter_mapping_reaches_both_ends(h, w, sh, sw):
    lo, hi = np.zeros(8, np.float32), np.full(8, R.U_MAX, np.float32)
    assert np.float32(R.U_MAX) == np.float32(0.99999994) and np.float32(R.U_MAX) < 1
    p0, p1 = R.params(lo, h, w, 7), R.params(hi, h, w, 7)
    assert (p0["ty"], p0["tx"], p1["ty"], p1["tx"]) == (-sh, -sw, sh, sw)
    assert (p0["oy"], p0["ox"], p1["oy"], p1["ox"]) == (0, 0, h, w)
    assert (p0["b"], p0["s"], p0["k"]) == (-0.5, 0.0, 0.5)
    assert abs(p1["b"] - 0.5) < 1e-7 and abs(p1["s"] - 2.0) < 2e-7 and abs(p1["k"] - 1.5) < 2e-7
    # every value in between is hit, none outside
    us = np.linspace(0, R.U_MAX, 4001).astype(np.float32)
    tys = {R.params(np.array([0, 0, 0, v, v, v, v, 0], np.float32), h, w, 7)["ty"] for v in us}
    oys = {R.params(np.array([0, 0, 0, v, v, v, v, 0], np.float32), h, w, 7)["oy"] for v in us}
    assert tys == set(range(-sh, sh + 1)) and oys == set(range(0, h + 1))


def test_translation_moves_pixels_and_fills_with_zeros():
    h, w = 8, 12
    x = torch.arange(1, h * w * 3 + 1, dtype=torch.float64).reshape(1, h, w, 3)
    u = np.full((1, 8), 0.5, np.float32)
    u[0, 3], u[0, 4] = R.U_MAX, 0.0                  # ty = +1, tx = -2
    y = R.diffaugment(x, u, R.TRANSLATION)
    assert torch.equal(y[0, :h - 1, 2:], x[0, 1:, :w - 2])
    assert bool((y[0, h - 1] == 0).all()) and bool((y[0, :, :2] == 0).all())


def test_adjoint_identity_and_support_of_the_restatement():
    rs = np.random.RandomState(1)
    h, w = 8, 12
    u = R.draws(5, 7)
    n = len(u)
    for policy in R.POLICIES:
        x = torch.from_numpy(rs.randn(n, h, w, 3)).requires_grad_(True)
        dy = torch.from_numpy(rs.randn(n, h, w, 3))
        y = R.diffaugment(x, u, policy)
        (dx,) = torch.autograd.grad((y * dy).sum(), x)
        y0 = R.diffaugment(torch.zeros_like(x), u, policy)
        lhs, rhs = float(((y - y0).detach() * dy).sum()), float((x.detach() * dx).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), policy
        if not policy & R.COLOR:
            sup = torch.from_numpy(R.support(u, h, w, policy))
            assert bool((dx[~sup] == 0).all()) and bool((dx[sup] != 0).all()), policy
