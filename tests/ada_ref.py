"""The adaptive augmentation probability as include/rcgan_hip.h defines it (rcgan_diffaugment_gated_fwd, rcgan_ada_update), restated
with numpy / torch: the reference of the CPU property tests and of the GPU tests.

The per-sample policy is formed from (gate_u, p, policy) with the strict float32 comparison of the definition; the sample is then
tests/diffaugment_ref.augment_one under that policy (float64, the adjoint by autograd).  The controller runs in np.float32, one
operation per statement, in the order the definition gives.
"""
import numpy as np
import torch

from tests import diffaugment_ref as R

GATE_BITS = (R.COLOR, R.TRANSLATION, R.CUTOUT)        # columns 0, 1, 2 of gate_u; column 3 is reserved
STATE = ("p", "sign_sum", "image_count", "steps", "r_last", "updates")


def sample_policy(gate_u, p, policy):
    """int32 [n]: policy & sum_t (gate_u[i][t] < p ? bit_t : 0), the comparison strict and in float32 (a NaN p: nothing)."""
    g = np.asarray(gate_u, np.float32)
    assert g.ndim == 2 and g.shape[1] == 4, g.shape
    p = np.float32(p)
    out = np.zeros(len(g), np.int32)
    for t, bit in enumerate(GATE_BITS):
        out |= np.where(g[:, t] < p, bit, 0).astype(np.int32)
    return (out & np.int32(policy)).astype(np.int32)


def diffaugment(x, u, gate_u, p, policy):
    """x [n, h, w, 3] torch, u [n, 8], gate_u [n, 4], p a scalar -> [n, h, w, 3]: every sample under its own policy."""
    u = np.asarray(u, np.float32)
    assert u.shape == (x.shape[0], 8), u.shape
    pol = sample_policy(gate_u, p, policy)
    return torch.stack([R.augment_one(x[i], u[i], int(pol[i])) for i in range(x.shape[0])])


def gate_rows(p=0.5):
    """Eight rows: every combination of the three gates below p / not below p; the rows that are "not below" alternate between
    a gate EXACTLY equal to p (not applied: the comparison is strict) and one above it.  Column 3 is filled with 0: reserved,
    and must not apply anything."""
    p = np.float32(p)
    below, above = np.float32(p * np.float32(0.5)), np.float32(min(float(p) * 1.5, R.U_MAX))
    rows = []
    for combo in range(8):
        r = np.zeros(4, np.float32)
        for t in range(3):
            r[t] = below if combo & (1 << t) else (p if (combo + t) % 2 == 0 else above)
        rows.append(r)
    return np.stack(rows)


def gates(m, p=0.5):
    """gate_u [m, 4]: gate_rows(p) repeated with a stride that is coprime to the draw list's periods."""
    g = gate_rows(p)
    return np.stack([g[(3 * i + i // 8) % 8] for i in range(m)]).astype(np.float32)


def sign(v):
    """(v > 0) - (v < 0) as float32: +-0 and NaN give 0, +-inf give +-1."""
    v = np.asarray(v, np.float32)
    return (v > 0).astype(np.float32) - (v < 0).astype(np.float32)


def scores(logits, labels=None):
    """The scores rcgan_ada_update reads: logits [n, ld] at the row's label (column 0 without labels); a row whose label lies
    outside [0, ld) counts as zero."""
    lg = np.asarray(logits, np.float32)
    n, ld = lg.shape
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    ok = (lab >= 0) & (lab < ld)
    return np.where(ok, lg[np.arange(n), np.where(ok, lab, 0)], np.float32(0)).astype(np.float32)


def new_state(p=0.0):
    s = np.zeros(8, np.float32)
    s[0] = p
    return s


def update(state, logits, labels, target, images, interval):
    """One rcgan_ada_update call on a float32[8] state -> the new state (a copy), every operation in float32."""
    s = np.array(state, np.float32)
    f = np.float32
    n = len(logits)
    s[1] = s[1] + f(sign(scores(logits, labels)).astype(np.float64).sum())     # (a sum of small integers: exact in any order)
    s[2] = s[2] + f(n)
    s[3] = s[3] + f(1)
    if s[3] == f(interval):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = f(s[1] / s[2])
            d = f(r - f(target))
            step = f(f(sign(d) * s[2]) / f(images))
            p = f(s[0] + step)
        s[0] = f(0) if np.isnan(p) else min(max(p, f(0)), f(1))      # (fminf(fmaxf(p, 0), 1): a NaN state restarts at 0)
        s[4] = r
        s[5] = s[5] + f(1)
        s[1] = s[2] = s[3] = f(0)
    return s
