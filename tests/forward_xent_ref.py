"""Restatement of the forward-corrected cross-entropy (Patrini et al. 2017) for the tests, in log-space: for a row of logits z with
noisy label y~ and confusion matrix C (C[y, y~] = P(noisy y~ | clean y)),

    L = -log( (softmax(z) . C)[y~] ) = logsumexp(z) - logsumexp(z + log C[:, y~]),
    post[y] = softmax(z)[y] C[y, y~] / (softmax(z) . C)[y~],        dL/dz = softmax(z) - post,

in numpy float64 (``forward_xent``) and as a differentiable PyTorch term (``forward_loss``) under the training step of
tests/classifier_ref.py.  The product never imports this module.

The rules of the kernel it is compared with: the loss is the mean over ALL rows; a row whose label is outside [0, K) or whose column
C[:, y~] has no positive entry contributes nothing and gets a zero gradient row, a zero posterior row and recovered = -1; recovered is
the arg-max of the posterior and n_correct counts arg-max(z) == y~, both with the lowest index on ties."""
import numpy as np
import torch

from tests import classifier_ref as R


def _logsumexp(a):
    """Over the last axis, float64; a row of -inf gives -inf (no warning, no nan)."""
    m = a.max(axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return m[..., 0] + np.log(np.exp(a - m).sum(axis=-1))


def forward_xent(z, labels, C, weight=1.0):
    """-> dict(loss, dlogits [R,K], posterior [R,K], recovered [R], n_correct, valid [R]) in float64; loss and dlogits carry ``weight``
    and the 1/R of the mean."""
    z = np.asarray(z, np.float64)
    C = np.asarray(C, np.float64)
    lab = np.asarray(labels, np.int64)
    rows, K = z.shape
    in_range = (lab >= 0) & (lab < K)
    safe = np.where(in_range, lab, 0)
    with np.errstate(divide="ignore"):
        logc = np.log(C[:, safe].T)                        # [R,K]: log C[y, y~_r]; -inf where the entry is zero
    valid = in_range & np.isfinite(logc).any(axis=1)
    lse = _logsumexp(z)
    t = np.where(valid[:, None], z + logc, 0.0)            # (placeholder rows are masked below)
    lse_c = _logsumexp(t)
    row_loss = np.where(valid, lse - lse_c, 0.0)
    post = np.where(valid[:, None], np.exp(t - lse_c[:, None]), 0.0)
    soft = np.exp(z - lse[:, None])
    dl = np.where(valid[:, None], soft - post, 0.0) * (weight / rows)
    recovered = np.where(valid, np.argmax(post, axis=1), -1)
    n_correct = int((in_range & (np.argmax(z, axis=1) == lab)).sum())
    return dict(loss=weight * float(row_loss.sum()) / rows, dlogits=dl, posterior=post, recovered=recovered, n_correct=n_correct, valid=valid)


def near_ties(post, rel=1e-4):
    """Rows whose two largest posteriors differ by less than ``rel`` of the larger, and the indices of those two entries [R,2]."""
    order = np.argsort(-post, axis=1, kind="stable")[:, :2]
    top = np.take_along_axis(post, order, axis=1)
    return (top[:, 0] - top[:, 1]) < rel * top[:, 0], order


# ---------------------------------------------------------------------------------------------------------------- PyTorch
def forward_loss(lg, labels, C):
    """mean over rows of -log((softmax(lg) . C)[label]), differentiable; C a tensor or an array [K,K]."""
    C = torch.as_tensor(np.asarray(C), dtype=lg.dtype)
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    logc = torch.log(C[:, lab].t())
    return (torch.logsumexp(lg, dim=1) - torch.logsumexp(lg + logc, dim=1)).mean()


def posterior(lg, labels, C):
    """softmax(lg)[y] C[y, label] renormalised over y, no gradient."""
    with torch.no_grad():
        C = torch.as_tensor(np.asarray(C), dtype=lg.dtype)
        lab = torch.as_tensor(np.asarray(labels), dtype=torch.long)
        return torch.softmax(lg + torch.log(C[:, lab].t()), dim=1)


def loss_and_grads(P, images_nhwc, labels, C, eps=R.BN_EPS):
    """classifier_ref.loss_and_grads with the forward-corrected term: -> (loss, batch accuracy against ``labels``, {name: gradient})."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    lg = R.logits(Q, images_nhwc, eps)
    loss = forward_loss(lg, labels, C)
    loss.backward()
    acc = float((lg.detach().argmax(1).numpy() == np.asarray(labels)).mean())
    return float(loss.detach()), acc, {k: v.grad for k, v in Q.items()}


def sgd_step(P, A, images_nhwc, labels, C, lr, momentum=0.9, weight_decay=1e-4, nesterov=False, eps=R.BN_EPS):
    """classifier_ref.sgd_step with the forward-corrected term."""
    loss, acc, G = loss_and_grads(P, images_nhwc, labels, C, eps)
    dec = set(R.decayed_names())
    for k in P:
        P[k], A[k] = R.momentum_update(P[k], G[k], A[k], lr, momentum, weight_decay, nesterov, k in dec)
    return loss, acc, G


def recover(P, images_nhwc, noisy, C, batch=1000, eps=R.BN_EPS):
    """Recovered labels and posteriors under the evaluator's protocol: ``batch`` images at a time, each batch on its own moments."""
    out = []
    with torch.no_grad():
        for lo in range(0, len(images_nhwc), batch):
            out.append(posterior(R.logits(P, images_nhwc[lo:lo + batch], eps), noisy[lo:lo + batch], C).numpy())
    post = np.concatenate(out, axis=0)
    return np.argmax(post, axis=1), post


# ---------------------------------------------------------------------------------------------------------------- kernel test cases
SHAPES = [(1, 2), (7, 10), (128, 100), (1000, 100), (33, 1024), (4101, 3)]      # the last: wavefronts loop past the 1024-workgroup cap
VARIANTS = ["one_coin", "dense", "sparse", "identity"]
NEAR_TIE_CAP = 0.02          # no case may excuse more than this share of its rows from the exact comparison of ``recovered``
# seeds of the confusion matrix moved off the default where the restatement alone would break that cap: three classes with a zero column
# leave matrices of zeros and ones, under which the deliberately tied maxima are tied posteriors too
SEED_SHIFT = {(4101, 3, "sparse"): 9}


def confusion_variant(kind, K, seed):
    """-> float64 [K,K] whose entries are float32 values (what the device holds), rows summing to 1 within float32 rounding.
    one_coin: C_ALPHA(0.6); dense: Dirichlet(0.3) rows; sparse: the same with about half the entries zeroed, the LAST column entirely zero
    (no class emits that label) and the rows renormalised; identity."""
    rs = np.random.RandomState(1000 + seed)
    if kind == "identity":
        C = np.eye(K)
    elif kind == "one_coin":
        C = ((1 - 0.6) / (K - 1)) * np.ones((K, K)) + (0.6 - (1 - 0.6) / (K - 1)) * np.eye(K)
    else:
        C = rs.dirichlet(0.3 * np.ones(K), size=K)
        if kind == "sparse":
            C = C * (rs.uniform(size=(K, K)) < 0.5)
            C[:, K - 1] = 0.0
            for i in np.flatnonzero(C.sum(axis=1) <= 0):
                C[i, i if i != K - 1 else 0] = 1.0
            C = C / C.sum(axis=1, keepdims=True)
        elif kind != "dense":
            raise ValueError(kind)
    return C.astype(np.float32).astype(np.float64)


def kernel_case(rows, cols, kind, bad_rows=True):
    """-> (logits float32 [rows,cols], labels int32 [rows], C): logits and labels of test_gpu_classifier_ops._xent_case (uniform on +-80,
    deliberate ties of the row maximum).  bad_rows: every 11th row from row 5 gets a label outside [0, cols) (cols and -3 in turn);
    the sparse variant also points every 7th row from row 2 at its all-zero column."""
    from tests.test_gpu_classifier_ops import _xent_case
    seed = rows * 7 + cols
    x, lab = _xent_case(rows, cols, seed)
    C = confusion_variant(kind, cols, seed + SEED_SHIFT.get((rows, cols, kind), 0))
    if kind == "sparse":
        lab[2::7] = cols - 1
        if rows == 1:
            lab[0] = cols - 1
    if bad_rows:
        lab[5::22] = cols
        lab[16::22] = -3
    return x, lab, C
