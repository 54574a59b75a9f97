"""Training the label classifier, CPU side: the float64 restatement the GPU tests compare against (tests/classifier_ref.py) is the
network the reference's graph describes, the trainer's variables are the asset's, and the GAN trainer's --label_classifier flag
checks its asset before it touches a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import classifier_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH = os.path.join(ROOT, "tests", "golden", "cifar_label_classifier_graph.json")
ASSET = os.path.join(ROOT, "robust-conditional-gan_amd", "assets", "cifar_label_classifier.npz")


def _asset_floats():
    z = np.load(ASSET)
    return {k: z[k] for k in z.files if z[k].dtype.kind == "f" and z[k].ndim > 0}


def test_restatement_is_the_reference_graph():
    """With the committed CIFAR-10 asset the restatement's softmax equals the interpreter of the reference's own node list (float64)
    to 1e-6 on 64 random 0..255 images, batch-norm epsilon taken from the asset."""
    from oracle import graph_interp as GI
    nodes, consts = GI.load_graph(GRAPH, ASSET)
    z = np.load(ASSET)
    eps = {float(z[k]) for k in z.files if k.endswith("batchnorm|add|y")}
    assert eps == {float(np.float32(1e-3))} and float(np.float32(1e-3)) != 1e-3
    x = np.random.RandomState(11).randint(0, 256, size=(64, 32, 32, 3))
    ref = GI.run(nodes, consts, {"resnet_test_batch": x}, "infer_softmax")
    P = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in _asset_floats().items()}
    got = R.softmax(P, x, eps=eps.pop())
    assert got.shape == (64, 10)
    err = np.abs(got - ref).max()
    print("restatement vs graph interpreter: max |softmax difference| %.3e" % err)
    assert err <= 1e-6, err


@pytest.mark.parametrize("K", [10, 20, 100])
def test_variables_are_the_assets(K):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.classifier import N_DECAYED, create_classifier_variables
    want = {k: v.shape for k, v in _asset_floats().items()}
    assert len(want) == 95
    want["fc|fc_weights"], want["fc|fc_bias"] = (64, K), (K,)
    specs = create_classifier_variables(0, K)
    got = {n: tuple(s) for n, s, _ in specs}
    assert len(specs) == 95 and got == want
    assert sum(n.endswith("|conv") for n in got) == 31 and sum(n.endswith("|gamma") for n in got) == 31 and sum(n.endswith("|beta") for n in got) == 31
    assert got == R.shapes(K)
    for n, s, init in specs:
        assert init.shape == tuple(s) and init.dtype == np.float32, n
        if n.endswith("|gamma"):
            assert (init == 1).all()
        elif n.endswith("|beta") or n == "fc|fc_bias":
            assert (init == 0).all()
    # the decayed variables (filters, dense weight) lead, as one launch of the optimiser assumes
    assert [n for n, _, _ in specs[:N_DECAYED]] == R.decayed_names()
    assert not any(n.endswith("|conv") or n == "fc|fc_weights" for n, _, _ in specs[N_DECAYED:])
    w = dict((n, i) for n, _, i in specs)
    f = w["conv3_4|conv2_in_block|conv"]
    assert abs(f.std() - np.sqrt(2.0 / (9 * 64))) < 0.05 * np.sqrt(2.0 / (9 * 64))           # He-normal, fan-out
    assert np.abs(w["fc|fc_weights"]).max() <= 0.125 and np.abs(w["fc|fc_weights"]).max() > 0.1
    again = dict((n, i) for n, _, i in create_classifier_variables(0, K))
    assert all((again[n] == w[n]).all() for n in w)
    assert not (dict((n, i) for n, _, i in create_classifier_variables(1, K))["conv0|conv"] == w["conv0|conv"]).all()


def test_label_classifier_flag_checks_the_class_count_without_a_gpu(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import train_cifar
    with pytest.raises(ValueError) as e:
        train_cifar.main(["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--dataset", "cifar100", "--synthetic",
                          "--label_classifier", ASSET])
    assert "10" in str(e.value) and "100" in str(e.value), str(e.value)
    from rcgan_amd.eval_cifar import asset_n_classes
    assert asset_n_classes(ASSET) == 10


@pytest.mark.parametrize("K", [10, 20, 100, 1000])
def test_balanced_label_lists(K):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.train_cifar import gen_acc_label_lists
    calls = gen_acc_label_lists(K, balanced=True)
    assert len(calls) == 10 and all(len(c) == 100 for c in calls)
    labels = np.concatenate(calls)
    assert labels.min() >= 0 and labels.max() < K
    counts = np.bincount(labels, minlength=K)
    assert counts.max() - counts.min() <= 1, (counts.min(), counts.max())
    assert all(list(c) == sorted(c) for c in calls)
    if K == 10:
        today = [label for label in range(10) for _ in range(10)]
        assert gen_acc_label_lists(10) == [today] * 10
        assert [list(c) for c in calls] == [today] * 10


def test_augment_restatement():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, size=(3, 3072)).astype(np.uint8)
    out, lab = R.augment(img, [5, 6, 7], [2, 0, 2], [[0, 0, 0], [1, -2, 0], [0, 0, 1]])
    nhwc = R.chw_to_nhwc(img)
    assert (out[0] == nhwc[2]).all() and list(lab) == [7, 5, 7]
    assert (out[1][1:, :30] == nhwc[0][:31, 2:]).all() and (out[1][0] == 0).all() and (out[1][:, 30:] == 0).all()
    assert (out[2] == nhwc[2][:, ::-1]).all()


def test_lr_schedule():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.train_classifier import lr_at
    assert [lr_at(s, 100, 0.1) for s in (0, 49, 50, 74, 75, 99)] == [0.1, 0.1, 0.1 * 0.1, 0.1 * 0.1, 0.1 * 0.01, 0.1 * 0.01]
