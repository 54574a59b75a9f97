"""The float64 numpy restatement of the MNIST label classifier (tests/mnist_classifier_ref.py) against PyTorch-CPU autograd, its
pooling tie rule on windows built by hand, the variables, and the flag checks of both command lines.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mnist_classifier_ref as R
from tests import philox_ref as P


def _variables(seed, K=10):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist_classifier import create_mnist_classifier_variables
    return create_mnist_classifier_variables(seed, K)


def _torch_loss_and_grads(V, x, labels, mask, scale):
    """relu -> max_pool2d(2) -> ..., the mask applied explicitly, float64 autograd."""
    Q = {k: torch.from_numpy(np.asarray(v, np.float64)).clone().requires_grad_(True) for k, v in V.items()}
    conv = lambda t, w, b: F.conv2d(t, w.permute(3, 2, 0, 1), b, padding=2)
    t = torch.from_numpy(np.asarray(x, np.float64)).reshape(-1, 28, 28, 1).permute(0, 3, 1, 2)
    t = F.max_pool2d(torch.relu(conv(t, Q["conv1|w"], Q["conv1|b"])), 2)
    t = F.max_pool2d(torch.relu(conv(t, Q["conv2|w"], Q["conv2|b"])), 2)
    flat = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)                   # NHWC order
    feat = torch.relu(flat @ Q["fc1|w"] + Q["fc1|b"])
    drop = feat * torch.from_numpy(np.asarray(mask, np.float64) * float(scale))
    logits = drop @ Q["fc2|w"] + Q["fc2|b"]
    loss = F.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.long))
    loss.backward()
    return float(loss.detach()), logits.detach().numpy(), feat.detach().numpy(), {k: v.grad.numpy() for k, v in Q.items()}


def test_restatement_against_torch_autograd():
    B, keep = 3, 0.5
    rs = np.random.RandomState(0)
    V = {n: i for n, _, i in _variables(3)}
    x = rs.uniform(0, 1, size=(B, 28, 28, 1))
    labels = rs.randint(10, size=B)
    mask = R.dropout_mask(77, 5, B * 1024, keep).reshape(B, 1024)
    assert 0.4 < mask.mean() < 0.6
    scale = R.dropout_scale(keep)
    loss, acc, G, t = R.loss_and_grads(V, x, labels, mask, scale)
    loss_t, logits_t, feat_t, G_t = _torch_loss_and_grads(V, x, labels, mask, scale)
    assert abs(loss - loss_t) <= 1e-12 * max(1.0, abs(loss_t))
    assert np.abs(t["logits"] - logits_t).max() <= 1e-12 * np.abs(logits_t).max()
    assert np.abs(t["feat"] - feat_t).max() <= 1e-12 * np.abs(feat_t).max()
    assert set(G) == set(G_t) == set(R.NAMES)
    for n in R.NAMES:
        assert G[n].shape == R.shapes()[n]
        assert np.abs(G_t[n]).max() > 0, n
        assert np.abs(G[n] - G_t[n]).max() <= 1e-11 * np.abs(G_t[n]).max(), n
    # without a mask the features pass unchanged
    assert (R.forward(V, x)["drop"] == R.forward(V, x)["feat"]).all()
    assert 0.0 <= acc <= 1.0


def test_pooling_gradient_goes_to_the_first_of_two_equal_maxima():
    """Windows in the order (0,0), (0,1), (1,0), (1,1): the equal positive maxima sit at (0,1) and (1,0) -> (0,1) takes the gradient,
    which is what PyTorch's max_pool2d does; a window that is all <= 0 takes none (relu)."""
    x = np.zeros((1, 2, 4, 1))
    x[0, :, 0:2, 0] = [[0.25, 0.75], [0.75, -1.0]]          # two equal positive maxima
    x[0, :, 2:4, 0] = [[-0.5, 0.0], [0.0, -0.25]]           # all <= 0 (two zeros tie for the maximum)
    dy = np.array([3.0, 5.0]).reshape(1, 1, 2, 1)
    y = R.relu_maxpool2(x)
    assert y.reshape(-1).tolist() == [0.75, 0.0]
    dx = R.relu_maxpool2_grad(x, dy)
    want = np.zeros_like(x)
    want[0, 0, 1, 0] = 3.0
    assert (dx == want).all(), dx[0, :, :, 0]
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(torch.relu(xt), 2).backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    got = xt.grad.permute(0, 2, 3, 1).numpy()
    assert (got[0, :, 0:2, 0] == want[0, :, 0:2, 0]).all(), got[0, :, :, 0]       # the tie: the same element
    assert (got[0, :, 2:4, 0] == 0).all()                                         # relu'(0) = 0 in PyTorch too
    # float32 and 16-bit-valued inputs keep their dtype: the device comparison is bit for bit
    assert R.relu_maxpool2(x.astype(np.float32)).dtype == np.float32
    assert R.relu_maxpool2_grad(x.astype(np.float32), dy.astype(np.float32)).dtype == np.float32


def test_window_order_round_trips():
    x = np.arange(2 * 4 * 6 * 3, dtype=np.float64).reshape(2, 4, 6, 3)
    w = R._windows(x)
    assert (w[1, 1, 2, 1] == [x[1, 2, 4, 1], x[1, 2, 5, 1], x[1, 3, 4, 1], x[1, 3, 5, 1]]).all()
    assert (R._unwindows(w) == x).all()


def test_dropout_mask_is_the_stream():
    keep = 0.9
    words = P.stream_words(1234, 7, 10)
    want = [((int(r) >> 8) / 2.0 ** 24) < float(np.float32(keep)) for r in words]
    assert R.dropout_mask(1234, 7, 10, keep).tolist() == want
    assert R.dropout_mask(1234, 7, 4099, 1.0).all()
    assert float(R.dropout_scale(0.5)) == 2.0 and R.dropout_scale(0.9).dtype == np.float32


@pytest.mark.parametrize("K", [10, 37])
def test_variable_shapes(K):
    specs = _variables(0, K)
    assert [n for n, _, _ in specs] == list(R.NAMES)
    for n, s, init in specs:
        assert tuple(s) == R.shapes(K)[n] == init.shape and init.dtype == np.float32
        if n.endswith("|b"):
            assert (init == np.float32(0.1)).all()
        else:
            assert np.abs(init).max() <= 0.2 + 1e-7 and 0.08 < init.std() < 0.1          # truncated at two standard deviations: std 0.088
    again = _variables(0, K)
    assert all((a[2] == b[2]).all() for a, b in zip(specs, again))
    assert not (specs[0][2] == _variables(1, K)[0][2]).all()


def test_train_mnist_classifier_flag_errors(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_mnist_classifier as T
    base = ["--synthetic", "--log_file", str(tmp_path / "log.txt"), "--out", str(tmp_path / "a.npz")]
    for bad, word in [(["--synthetic"], "log_file"), (["--synthetic", "--log_file", "x"], "out"), (base + ["--alpha", "0"], "alpha"),
                      (base + ["--alpha", "1.5"], "alpha"), (base + ["--keep_prob", "0"], "keep_prob"), (base + ["--keep_prob", "1.01"], "keep_prob"),
                      (base + ["--loss", "hinge"], "loss"), (base + ["--loss", "forward"], "confusion_matrix"),
                      (base + ["--confusion_matrix", "known"], "forward"), (base + ["--recover_out", "r.npz"], "forward"),
                      (base + ["--loss", "forward", "--confusion_matrix", "estimate"], "estimate"),
                      (base + ["--loss", "forward", "--confusion_matrix", "c.txt"], "confusion_matrix")]:
        with pytest.raises(ValueError) as e:
            T.main(bad)
        assert word in str(e.value), (bad, str(e.value))
    f = T.define_flags().parse([])
    assert f.lr == 1e-4 and f.keep_prob == 0.5 and f.batch_size == 128 and f.loss == "ce" and f.confusion_matrix is None


def test_train_mnist_label_classifier_flag(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_mnist
    assert train_mnist.define_flags().parse([]).label_classifier is None
    asset = str(tmp_path / "clf.npz")
    np.savez(asset, **{n: i for n, _, i in _variables(0, 10)})
    common = ["--train", "--synthetic", "--checkpoint_dir", str(tmp_path / "ck")]
    with pytest.raises(ValueError) as e:          # both classifiers: an error before any GPU work (and before any directory is made)
        train_mnist.main(common + ["--label_classifier", asset, "--label_classifier_fn", "rcgan_amd.eval_mnist:template_predict"])
    assert "label_classifier_fn" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        train_mnist.main(common + ["--label_classifier", str(tmp_path / "missing.npz")])
    assert "missing" in str(e.value)
    np.savez(str(tmp_path / "clf7.npz"), **{n: i for n, _, i in _variables(0, 7)})
    with pytest.raises(ValueError) as e:
        train_mnist.main(common + ["--label_classifier", str(tmp_path / "clf7.npz")])
    assert "7 classes" in str(e.value)
    assert not (tmp_path / "ck").exists()
