"""Noise-robust label classifier, CPU side: the float64 restatement of the forward-corrected loss the GPU tests compare against
(tests/forward_xent_ref.py) against autograd, the host helpers that corrupt labels and estimate the confusion matrix, and the flags of
train_classifier."""
import numpy as np
import pytest
import torch

from tests import forward_xent_ref as FR


def _random_C(rs, K, zeros=False):
    C = rs.dirichlet(0.5 * np.ones(K), size=K)
    if zeros:
        C = C * (rs.uniform(size=(K, K)) < 0.6) + 0.05 * np.eye(K)
        C /= C.sum(axis=1, keepdims=True)
    return C


@pytest.mark.parametrize("rows,K,zeros", [(5, 2, False), (33, 10, False), (64, 100, True), (17, 7, True)])
def test_restatement_against_autograd(rows, K, zeros):
    """Loss, gradient and posterior of the log-space restatement equal float64 autograd of -log((softmax(z) . C)[label]), written as it
    reads, to 1e-12; posterior rows sum to 1."""
    rs = np.random.RandomState(rows + K)
    z = rs.randn(rows, K) * 4
    lab = rs.randint(K, size=rows)
    C = _random_C(rs, K, zeros)
    if zeros:
        lab = np.array([int(rs.choice(np.flatnonzero(C.sum(0) > 0))) for _ in range(rows)])
    weight = 0.75
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    mixed = torch.softmax(zt, dim=1) @ torch.tensor(C, dtype=torch.float64)               # [rows, K]: P(noisy | x)
    loss = weight * (-torch.log(mixed[torch.arange(rows), torch.as_tensor(lab)])).mean()
    loss.backward()
    post_ref = (torch.softmax(zt, dim=1) * torch.tensor(C[:, lab].T)).detach().numpy()
    post_ref /= post_ref.sum(axis=1, keepdims=True)
    got = FR.forward_xent(z, lab, C, weight)
    assert got["valid"].all()
    assert abs(got["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.abs(got["dlogits"] - zt.grad.numpy()).max() <= 1e-12
    assert np.abs(got["posterior"] - post_ref).max() <= 1e-12
    assert np.abs(got["posterior"].sum(axis=1) - 1.0).max() <= 1e-12
    assert (got["recovered"] == np.argmax(post_ref, axis=1)).all()
    # the differentiable term the step restatement trains with is the same function
    zt2 = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    l2 = weight * FR.forward_loss(zt2, lab, C)
    l2.backward()
    assert abs(float(l2.detach()) - float(loss.detach())) <= 1e-12 and np.abs(zt2.grad.numpy() - zt.grad.numpy()).max() <= 1e-12
    assert np.abs(FR.posterior(zt2.detach(), lab, C).numpy() - post_ref).max() <= 1e-12


def test_restatement_with_identity_is_plain_cross_entropy():
    rs = np.random.RandomState(3)
    z = rs.uniform(-80, 80, size=(40, 13))
    lab = rs.randint(13, size=40)
    zt = torch.tensor(z, requires_grad=True)
    ce = torch.nn.functional.cross_entropy(zt, torch.as_tensor(lab))
    ce.backward()
    got = FR.forward_xent(z, lab, np.eye(13))
    assert abs(got["loss"] - float(ce.detach())) <= 1e-12 * abs(float(ce.detach()))
    assert np.abs(got["dlogits"] - zt.grad.numpy()).max() <= 1e-12
    assert (got["posterior"] == np.eye(13)[lab]).all() and (got["recovered"] == lab).all()
    assert got["n_correct"] == int((np.argmax(z, 1) == lab).sum())


def test_restatement_rows_without_support_or_label():
    """A label outside [0, K) or a label no class emits: no loss, zero gradient and posterior rows, recovered -1; the mean still runs
    over all rows."""
    rs = np.random.RandomState(4)
    z = rs.randn(6, 4)
    C = np.array([[0.5, 0.5, 0, 0], [0, 1.0, 0, 0], [0.25, 0.75, 0, 0], [0, 0.5, 0, 0.5]])
    lab = np.array([0, 1, 2, 3, 4, -1])                  # column 2 is all zero
    got = FR.forward_xent(z, lab, C)
    assert list(got["valid"]) == [True, True, False, True, False, False]
    for r in (2, 4, 5):
        assert (got["dlogits"][r] == 0).all() and (got["posterior"][r] == 0).all() and got["recovered"][r] == -1
    only = FR.forward_xent(z[[0, 1, 3]], lab[[0, 1, 3]], C)
    assert abs(got["loss"] * 6 - only["loss"] * 3) <= 1e-12
    assert np.abs(got["dlogits"][[0, 1, 3]] * 6 - only["dlogits"] * 3).max() <= 1e-12
    assert got["posterior"][3, 0] == 0 and got["posterior"][3, 2] == 0       # classes that cannot emit label 3


@pytest.mark.parametrize("rows,cols", FR.SHAPES)
@pytest.mark.parametrize("kind", FR.VARIANTS)
def test_kernel_cases_keep_the_near_tie_cap(rows, cols, kind):
    """The cases of tests/test_gpu_forward_xent.py: on the restatement alone, at most 2 % of a case's rows have their two largest
    posteriors within 1e-4 of each other (the rows whose ``recovered`` may be either of the two)."""
    x, lab, C = FR.kernel_case(rows, cols, kind)
    assert np.abs(C.sum(axis=1) - 1.0).max() <= 1e-6 and C.min() >= 0
    ref = FR.forward_xent(x, lab, C, 0.75)
    near, _ = FR.near_ties(ref["posterior"])
    assert (near & ref["valid"]).mean() <= FR.NEAR_TIE_CAP
    if kind == "sparse":
        assert (C[:, cols - 1] == 0).all() and (lab == cols - 1).any()
    if rows >= 7:
        assert (~ref["valid"]).any() and ((lab < 0) | (lab >= cols)).any()


# ------------------------------------------------------------------------------------------------ host helpers
def test_noisy_labels_is_deterministic_and_follows_C():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    K, n = 10, 50000
    rs = np.random.RandomState(5)
    labels = rs.randint(K, size=n)
    C = rs.dirichlet(0.7 * np.ones(K), size=K)
    C[3] = 0
    C[3, 6] = 1.0                                        # a deterministic row, and zeros that must never be drawn
    C[4, :5] = 0
    C[4] /= C[4].sum()
    a = D.noisy_labels(labels, C, np.random.RandomState(11))
    b = D.noisy_labels(labels, C, np.random.RandomState(11))
    c = D.noisy_labels(labels, C, np.random.RandomState(12))
    assert a.shape == (n,) and (a == b).all() and not (a == c).all()
    assert a.min() >= 0 and a.max() < K
    for i in range(K):
        ni = int((labels == i).sum())
        freq = np.bincount(a[labels == i], minlength=K) / ni
        se = np.sqrt(C[i] * (1 - C[i]) / ni)
        assert (np.abs(freq - C[i]) <= 4 * se).all(), (i, freq, C[i])          # (se = 0 where C is 0 or 1: those must be exact)
    one_coin = D.noisy_labels(labels, D.C_ALPHA(0.6, K), np.random.RandomState(0))
    assert abs((one_coin == labels).mean() - 0.6) <= 4 * np.sqrt(0.24 / n)
    assert (D.noisy_labels(labels, np.eye(K), np.random.RandomState(0)) == labels).all()
    with pytest.raises(ValueError):
        D.noisy_labels(labels, 0.5 * np.eye(K), rs)
    with pytest.raises(ValueError):
        D.noisy_labels(labels + 1, np.eye(K), rs)


def test_anchor_estimate_returns_C_on_perfect_anchors():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    K = 6
    rs = np.random.RandomState(9)
    C = 0.5 * np.eye(K) + 0.5 * rs.dirichlet(np.ones(K), size=K)          # each diagonal entry >= 0.5: the largest of its column
    assert all(C[i, i] == C[:, i].max() for i in range(K))
    p_clean = rs.dirichlet(0.3 * np.ones(K), size=500)
    at = rs.choice(500, K, replace=False)
    p_clean[at] = np.eye(K)                                                 # one exact one-hot row per class, scattered
    probs = p_clean @ C
    got = D.estimate_confusion_anchor(probs, quantile=1.0)
    assert (got == C).all()
    # below 1 the estimate comes from a less extreme sample: still close for well-separated classes, and it is some sample's row
    q = D.estimate_confusion_anchor(probs, quantile=0.97)
    assert q.shape == (K, K) and all(any((q[i] == probs[j]).all() for j in range(500)) for i in range(K))
    for i in range(K):
        assert q[i, i] <= got[i, i] and q[i, i] >= np.sort(probs[:, i])[int(0.97 * 499)] - 1e-15
    with pytest.raises(ValueError):
        D.estimate_confusion_anchor(probs, quantile=0.0)
    with pytest.raises(ValueError):
        D.estimate_confusion_anchor(probs[0], quantile=1.0)


def test_confusion_matrix_validation():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    assert (D.check_confusion_matrix(D.C_ALPHA(0.6, 20), 20) == D.C_ALPHA(0.6, 20)).all()
    bad_sum, negative = np.eye(4), np.eye(4)
    bad_sum[0, 0] = 1 + 1e-5
    negative[0, :2] = (1.25, -0.25)
    for bad, K in ((bad_sum, 4), (negative, 4), (np.eye(4), 5), (np.eye(4)[:3], 4)):
        with pytest.raises(ValueError):
            D.check_confusion_matrix(bad, K)


# ------------------------------------------------------------------------------------------------ flags
def test_default_flags_are_todays():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_classifier as T
    F = T.define_flags().parse(["--log_file", "l", "--out", "o"])
    today = dict(dataset="cifar", coarse_labels=False, synthetic=False, synthetic_kind="uniform", synthetic_samples=50000, epochs=160,
                 max_steps=0, batch_size=128, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=False, no_augment=False, seed=0,
                 f32_matmul_precision="highest", out="o", log_file="l")
    for k, v in today.items():
        assert getattr(F, k) == v, k
    assert F.alpha == 1.0 and F.loss == "ce" and F.confusion_matrix is None and F.recover_out is None and F.label_seed == 0
    assert F.estimate_steps == 0 and F.anchor_quantile == 0.97
    assert T.check_noise_flags(F) is None                 # plain cross-entropy on the labels as they are


@pytest.mark.parametrize("argv,word", [
    (["--loss", "forward"], "confusion_matrix"),
    (["--loss", "backward", "--confusion_matrix", "known"], "loss"),
    (["--confusion_matrix", "known"], "forward"),
    (["--recover_out", "r.npz"], "forward"),
    (["--loss", "forward", "--confusion_matrix", "guess"], "confusion_matrix"),
    (["--alpha", "0"], "alpha"),
    (["--alpha", "1.5"], "alpha"),
    (["--loss", "forward", "--confusion_matrix", "estimate", "--anchor_quantile", "1.5"], "anchor_quantile"),
    (["--loss", "forward", "--confusion_matrix", "estimate", "--estimate_steps", "-1"], "estimate_steps"),
])
def test_flag_errors_come_before_any_work(tmp_path, argv, word):
    """main() refuses an inconsistent set of noise flags before it loads data or touches a GPU."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_classifier as T
    with pytest.raises(ValueError) as e:
        T.main(["--log_file", str(tmp_path / "log.txt"), "--out", str(tmp_path / "a.npz"), "--synthetic"] + argv)
    assert word in str(e.value), str(e.value)
    assert not (tmp_path / "log.txt").exists() and not (tmp_path / "a.npz").exists()


def test_accepted_flag_combinations():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_classifier as T
    parse = lambda a: T.check_noise_flags(T.define_flags().parse(a))
    assert parse(["--alpha", "0.6"]) is None                                             # the baseline: plain cross-entropy on noisy labels
    assert parse(["--alpha", "0.6", "--loss", "forward", "--confusion_matrix", "known", "--recover_out", "r.npz"]) == "known"
    assert parse(["--alpha", "0.6", "--loss", "forward", "--confusion_matrix", "estimate", "--estimate_steps", "100"]) == "estimate"
    assert parse(["--loss", "forward", "--confusion_matrix", "runs/C.npy"]) == "runs/C.npy"
