"""float64 numpy restatement of the LeCam regulariser as include/rcgan_hip.h defines it (no GPU, no torch):

  loss_reg_fwd_bwd   one loss part with the term: per logit x, t = loss_kind(x) + lam (x - a)^2 and dt/dx = loss_kind'(x) + 2 lam (x - a)
                     under the gate, weighted as the part's loss term is weighted (all elements equally, or mean_rows sum_cols w);
  scores / update    rcgan_lecam_update: the two batch means of the parts' scores and the anchors' exponential moving averages.

Every sum comes with its ``mag`` (the sum of the absolute values of its terms) for tests/head_loss_ref.py's ``sum_bound``.
"""
import numpy as np

from tests import head_loss_ref as R

A_REAL, A_FAKE, UPDATES, MEAN_REAL, MEAN_FAKE, SKIPPED = 0, 1, 2, 3, 4, 5
EPS32 = R.EPS32


def f64(a):
    return np.asarray(a, np.float64)


def gate_open(lam, gate):
    """The term is on iff lambda != 0 and the gate word (None: no gate) is > 0."""
    return lam != 0 and (gate is None or float(gate) > 0)


def loss_reg_fwd_bwd(kind, x, wts, weight, lam, anchor, gate=None, scale=1.0):
    """x [rows, cols] (or [rows]); wts None or [rows, cols].  -> dict:
      value, mag      weight * (L + lam R) and the sum of |terms| behind it
      R, R_mag        the unweighted R of the part (0 with the term off)
      dlogit, dlogit_mag   scale * weight * wf * (loss' + 2 lam (x - a)) and scale * |weight wf| * (|loss'| + |2 lam (x - a)|)
      dwts            scale * weight * (loss + lam (x - a)^2) / rows
    """
    x = f64(x)
    if x.ndim == 1:
        x = x[:, None]
    rows = x.shape[0]
    t, d = R.loss_term(kind, x)
    wf = f64(wts) / rows if wts is not None else np.full(x.shape, 1.0 / x.size)
    on = gate_open(lam, gate)
    u = x - float(anchor) if on else np.zeros_like(x)
    q = u * u
    lam = float(lam) if on else 0.0
    tt, dd = t + lam * q, d + 2.0 * lam * u
    terms = weight * tt * wf
    rterms = q * wf
    return dict(value=terms.sum(), mag=(np.abs(weight * t * wf) + np.abs(weight * lam * q * wf)).sum(),
                R=rterms.sum(), R_mag=np.abs(rterms).sum(),
                dlogit=scale * weight * dd * wf, dlogit_mag=np.abs(scale * weight * wf) * (np.abs(d) + np.abs(2.0 * lam * u)),
                dwts=scale * weight * tt / rows, dwts_mag=np.abs(scale * weight / rows) * (np.abs(t) + np.abs(lam * q)))


def scores(logits, labels=None, wts=None):
    """The score of every row and its mag: the logit itself (one column), the logit at the label (0 for a label outside the row), or
    sum_l w[s, l] logit[s, l]."""
    lg = f64(logits)
    if lg.ndim == 1:
        lg = lg[:, None]
    n, ld = lg.shape
    assert labels is None or wts is None
    if wts is not None:
        pr = f64(wts) * lg
        return pr.sum(1), np.abs(pr).sum(1)
    if labels is None:
        assert ld == 1
        return lg[:, 0].copy(), np.abs(lg[:, 0])
    lab = np.asarray(labels, np.int64)
    ok = (lab >= 0) & (lab < ld)
    s = np.zeros(n)
    s[ok] = lg[np.arange(n)[ok], lab[ok]]
    return s, np.abs(s)


def batch_mean(logits, labels=None, wts=None):
    """-> mean of the scores over ALL rows, its mag (sum |terms| / rows), the number of terms added."""
    with np.errstate(invalid="ignore", over="ignore"):
        s, mag = scores(logits, labels, wts)
        cols = np.shape(logits)[1] if (wts is not None and np.ndim(logits) > 1) else 1
        return s.sum() / len(s), mag.sum() / len(s), len(s) * cols


def new_state():
    return np.zeros(8, np.float64)


def update(state, mean_real, mean_fake, decay):
    """One rcgan_lecam_update on a float64 copy of the state, from the two batch means."""
    st = f64(state).copy()
    if not (np.isfinite(mean_real) and np.isfinite(mean_fake)):
        st[SKIPPED] += 1
        return st
    if st[UPDATES] == 0:
        st[A_REAL], st[A_FAKE] = mean_real, mean_fake
    else:
        st[A_REAL] = decay * st[A_REAL] + (1.0 - decay) * mean_real
        st[A_FAKE] = decay * st[A_FAKE] + (1.0 - decay) * mean_fake
    st[UPDATES] += 1
    st[MEAN_REAL], st[MEAN_FAKE] = mean_real, mean_fake
    return st


def update_from_logits(state, logits, rows_a, decay, part_a=(None, None), part_b=(None, None)):
    """rcgan_lecam_update on logits [rows_a + rows_b, ld]; part_x = (labels, wts).  -> new state, (mean bound a, mean bound b): the
    forward bounds (terms + 4) 2^-24 sum|terms| / rows of the two fp32 means."""
    lg = f64(logits)
    if lg.ndim == 1:
        lg = lg[:, None]
    ma, mag_a, na = batch_mean(lg[:rows_a], *part_a)
    mb, mag_b, nb = batch_mean(lg[rows_a:], *part_b)
    return update(state, ma, mb, decay), ((na + 4) * EPS32 * mag_a, (nb + 4) * EPS32 * mag_b)
