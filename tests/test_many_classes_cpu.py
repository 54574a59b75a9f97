"""Host side of the K-class models (CIFAR-100): confusion matrices, label noise, the CIFAR-100 loader, the trainer's --dataset flag
and the class-count bounds.  No GPU needed."""
import pickle

import numpy as np
import pytest


def _old_c_alpha(alpha):
    return ((1 - alpha) / 9.0) * np.ones((10, 10)) + (alpha - (1 - alpha) / 9.0) * np.eye(10)


def _old_corrupt(labels, C, rng):
    labels = np.array(labels)
    labels_random = rng.randint(10, size=50000)
    labels_biased = np.zeros((50000,))
    labels_inv_weights = np.zeros((50000, 10))
    C_inv = np.linalg.inv(C)
    for i in range(len(labels)):
        labels[i] = np.flatnonzero(rng.multinomial(1, C[labels[i], :]))[0]
        labels_inv_weights[i] = C_inv[labels[i], :]
        labels_biased[i] = np.flatnonzero(rng.multinomial(1, C[labels_random[i], :]))[0]
    return labels, labels_random, labels_biased, labels_inv_weights


@pytest.mark.parametrize("alpha", [0.0, 0.2, 0.6, 1.0, 0.37])
def test_c_alpha_ten_classes_bit_identical(alpha):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar, data
    ref = _old_c_alpha(alpha)
    for f in (cifar.C_ALPHA, data.C_ALPHA):
        assert np.array_equal(f(alpha), ref) and np.array_equal(f(alpha, 10), ref)


def test_corrupt_labels_ten_classes_same_stream():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data
    labels = np.random.RandomState(1).randint(10, size=2000)
    C = data.C_ALPHA(0.6)
    a = data.corrupt_labels(labels, C, np.random.RandomState(7))
    b = _old_corrupt(labels, C, np.random.RandomState(7))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_hundred_classes_noise():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data
    K, alpha, n = 100, 0.6, 5000
    C = data.C_ALPHA(alpha, K)
    assert C.shape == (K, K)
    assert np.allclose(C.sum(1), 1.0, atol=1e-12)
    assert np.allclose(np.diag(C), alpha) and np.allclose(C[0, 1], (1 - alpha) / 99)
    clean = np.random.RandomState(2).randint(K, size=n)
    noisy, rnd, bia, inv = data.corrupt_labels(clean, C, np.random.RandomState(3), n_classes=K)
    assert rnd.max() < K and inv.shape == (50000, K)
    flips = float(np.mean(noisy != clean))
    sd = np.sqrt(alpha * (1 - alpha) / n)
    assert abs(flips - (1 - alpha)) <= 4 * sd, flips           # binomial bounds of the flip rate
    assert np.allclose(inv[:n], np.linalg.inv(C)[noisy])
    with pytest.raises(ValueError):
        data.corrupt_labels(clean, C, np.random.RandomState(3), n_classes=10)


@pytest.mark.parametrize("coarse", [False, True])
def test_cifar100_loader(tmp_path, coarse):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data
    rs = np.random.RandomState(5)
    for name, n in (("train", 40), ("test", 20)):
        d = {b"data": rs.randint(0, 256, size=(n, 3072)).astype(np.uint8), b"fine_labels": list(rs.randint(100, size=n)),
             b"coarse_labels": list(rs.randint(20, size=n)), b"filenames": [b"x"] * n}
        with open(tmp_path / name, "wb") as f:
            pickle.dump(d, f)
    x, y = data.unpickle100(str(tmp_path / "train"), coarse)
    with open(tmp_path / "train", "rb") as f:
        raw = pickle.load(f, encoding="bytes")
    assert np.array_equal(x, raw[b"data"]) and list(y) == raw[b"coarse_labels" if coarse else b"fine_labels"]
    K = 20 if coarse else 100
    train, dev = data.load100(8, str(tmp_path), data.C_ALPHA(0.6, K), np.random.RandomState(0), coarse=coarse)
    batches = list(train())
    assert len(batches) == 5 and len(list(dev())) == 2
    img, lab, rnd, bia, inv = batches[0]
    assert img.shape == (8, 3072) and inv.shape == (8, K) and lab.max() < K and rnd.max() < K
    with pytest.raises(ValueError):
        data.load100(8, str(tmp_path), data.C_ALPHA(0.6, 10), coarse=coarse)


def test_synthetic_templates_for_many_classes():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data
    t10, t100 = data.class_templates(), data.class_templates(100)
    assert t100.shape == (100, 3, 32, 32) and np.array_equal(t100[:10], t10)
    x, y = data.synthetic_cifar(50, 1, "templates", n_classes=100)
    assert x.shape == (50, 3072) and y.max() < 100
    a, b = data.synthetic_cifar(50, 1, "templates"), data.synthetic_cifar(50, 1, "templates", n_classes=10)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_dataset_flag():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar as T
    parse = lambda *a: T.define_flags().parse(list(a))
    assert T.dataset_setup(parse()) == (10, T.DATA_DIR)
    assert T.dataset_setup(parse("--dataset", "cifar100")) == (100, T.DATA_DIR_100)
    assert T.dataset_setup(parse("--dataset", "cifar100", "--coarse_labels")) == (20, T.DATA_DIR_100)
    assert T.dataset_setup(parse("--dataset", "cifar100", "--data_dir", "/x")) == (100, "/x")
    with pytest.raises(ValueError, match="unknown --dataset"):
        T.dataset_setup(parse("--dataset", "mnist"))
    with pytest.raises(ValueError, match="unknown --dataset"):
        T.main(["--dataset", "svhn", "--log_file", "/nonexistent/x.log"])
    assert np.array_equal(T.grid_labels(10), np.array([k for k in range(10) for _ in range(10)]))
    assert np.array_equal(T.grid_labels(100), np.arange(100))


@pytest.mark.parametrize("k", [1, 1025, 0, 2.5])
def test_class_count_rejected_before_any_context(k, monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar, runtime

    def no_context(*a, **kw):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cifar, "Context", no_context)
    monkeypatch.setattr(runtime, "Context", no_context)
    with pytest.raises(ValueError, match="n_classes"):
        cifar.CifarRCGAN(n_classes=k)
    with pytest.raises(ValueError, match="n_classes"):
        cifar.create_variables(0, n_classes=k)


def test_variables_sized_by_class_count():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar
    ref = cifar.create_variables(0, "rcgan-u", True, "linear", True, 0.2)
    same = cifar.create_variables(0, "rcgan-u", True, "linear", True, 0.2, n_classes=10)
    for a, b in zip(ref[:3], same[:3]):
        for (n1, s1, v1), (n2, s2, v2) in zip(a, b):
            assert n1 == n2 and s1 == s2 and np.array_equal(v1, v2)
    gs, ds, cs, U = cifar.create_variables(0, "rcgan-u", True, "linear", True, 0.2, n_classes=100)
    shapes = {n: s for n, s, _ in gs + ds + cs}
    assert shapes["Generator/G.Block.1.N1/CondBatchNorm/scale"] == (100, 1024)
    assert shapes["Discriminator/Embedding.Label/embedding_map"] == (100, 300)
    assert shapes["Discriminator/D.d_perm_classifier_h1/W"] == (3072, 100)
    assert shapes["confusion_logits"] == (100, 100)
    m = cifar.confusion_logits_initial(True, 0.995, np.random.RandomState(0), 10)
    assert np.array_equal(m, cifar.confusion_logits_initial(True, 0.995, np.random.RandomState(0)))
    assert m[0, 0] == np.float32(7.0 - 0.7)
