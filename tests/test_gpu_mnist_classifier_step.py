"""A training step of the MNIST label classifier on the engine against the float64 restatement (tests/mnist_classifier_ref.py) with
the mask the device stream draws, the Adam update on the engine's own gradient, the captured step against the eager one, the
forward-corrected loss at C = I against the plain one, and the way out: the asset MnistLabelClassifier reads and the checkpoint."""
import numpy as np
import pytest
import torch

from tests import mnist_classifier_ref as R
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu
B, N, KEEP, LR = 8, 32, 0.5, 1e-3
# No pre-activation of the float64 reference (both convolution outputs, the dense layer in front of the features) may sit closer to
# zero than this, and no pooling window may hold its two largest values closer together: at such a point float32 and float64
# legitimately take different branches and one flipped element moves a whole gradient column (tests/test_gpu_classifier_step.py).
KINK_MARGIN = 5e-6
DATA_SEED = 1          # the first of 0, 1, 2, ... whose batch keeps that margin (seed 0: 3.2e-7, seed 1: 5.35e-6); asserted in the test


def _data(seed):
    rs = np.random.RandomState(seed)
    images = rs.uniform(0, 1, size=(N, 784)).astype(np.float32)
    labels = rs.randint(10, size=N)
    steps = [rs.randint(N, size=B).astype(np.int32) for _ in range(5)]
    return images, labels, steps


def _variables(seed):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist_classifier import create_mnist_classifier_variables
    return create_mnist_classifier_variables(seed)


def _trainer(variables, images, labels, use_graphs, confusion_matrix=None):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist_classifier import MnistClassifierTrainer
    t = MnistClassifierTrainer(batch_size=B, keep_prob=KEEP, use_graphs=use_graphs, variables=variables, confusion_matrix=confusion_matrix)
    t.load_data(images, labels)
    return t


def _slabs(t):
    with torch.cuda.stream(t.ctx.stream):
        out = [s.cpu().numpy() for s in (t.P.value, t.P.m, t.P.v)]
    t.ctx.sync()
    return [s.view(np.uint32) for s in out]


def test_training_step_against_float64_and_its_adam_update():
    """Batch 8, keep_prob 0.5, data seed 1 (the first whose float64 reference keeps KINK_MARGIN: 5.35e-6).  Loss within
    2e-5 max(1, |L|), each of the eight gradients within 1e-2 of its own scale; then every variable equals TF-Adam evaluated on the
    engine's own downloaded gradient to 2.5e-7 of the weight scale (tests/test_gpu_fullbatch_steps.py)."""
    images, labels, steps = _data(DATA_SEED)
    variables = _variables(DATA_SEED)
    V = {n: i for n, _, i in variables}
    index = steps[0]
    t = _trainer(variables, images, labels, use_graphs=False)
    try:
        assert t.rng_offset() == 0
        mask = R.dropout_mask(t.dropout_seed, 0, B * 1024, KEEP).reshape(B, 1024)
        loss_ref, acc_ref, G, tr = R.loss_and_grads(V, images[index], labels[index], mask, R.dropout_scale(KEEP))
        nearest = R.nearest_kink(tr)
        print("nearest kink of the float64 reference: %.3e" % nearest)
        assert nearest >= KINK_MARGIN, "a reference value %.1e from a kink: the comparison is ill-posed" % nearest
        t.step(LR, index=index)
        loss, acc = t.losses()
        got = t.get_grads()
        assert t.rng_offset() == B * 1024 // 4
        errs = {n: float(np.abs(got[n] - G[n]).max() / (np.abs(G[n]).max() + 1e-12)) for n in R.NAMES}
        print("loss %.7f (float64 %.7f, diff %.2e), batch accuracy %.3f (%.3f)" % (loss, loss_ref, abs(loss - loss_ref), acc, acc_ref))
        print("gradient error relative to its own scale: %s" % {n: "%.2e" % e for n, e in errs.items()})
        assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
        assert set(got) == set(R.NAMES)
        for n in R.NAMES:
            assert np.abs(G[n]).max() > 0, n
            assert_close(got[n], G[n], 1e-2, "gradient of " + n)
        worst = 0.0
        for n in R.NAMES:
            w1, m1, v1 = R.adam_np(V[n], got[n].astype(np.float32), np.zeros_like(V[n]), np.zeros_like(V[n]), 1, LR)
            d = float(np.abs(t.P.get(n) - w1).max()) / max(1.0, float(np.abs(w1).max()))
            worst = max(worst, d)
            assert d <= 2.5e-7, "Adam update of %s: max difference %.3e (one fp32 ulp of the weight scale = 1.2e-7)" % (n, d)
            assert np.abs(t.P.get(n) - V[n]).max() > 0, n
        print("worst Adam difference %.3e of the weight scale" % worst)
    finally:
        t.close()


def test_captured_steps_equal_eager_steps_bit_for_bit():
    images, labels, steps = _data(3)
    variables = _variables(3)
    eager = _trainer(variables, images, labels, use_graphs=False)
    graph = _trainer(variables, images, labels, use_graphs=True)
    try:
        # the captured trainer rehearses its first step eagerly, captures the second and replays from then on: four steps give three
        # that ran from the graph.  Masks follow the device stream in both.
        for k, index in enumerate(steps[:4]):
            lr = LR if k < 3 else 0.1 * LR
            eager.step(lr, index=index)
            graph.step(lr, index=index)
            for a, b, what in zip(_slabs(eager), _slabs(graph), ("value", "m", "v")):
                assert (a == b).all(), "step %d: %s" % (k, what)
            assert eager.losses() == graph.losses()
            assert eager.rng_offset() == graph.rng_offset() == (k + 1) * B * 1024 // 4
        assert graph._graph is not None and eager._graph is None
    finally:
        eager.close()
        graph.close()


def test_identity_confusion_matrix_is_plain_cross_entropy_bit_for_bit():
    """The promise of rcgan_softmax_xent_forward_fwd_bwd's header, through two whole steps; and label recovery under C = I returns the
    given labels."""
    images, labels, steps = _data(4)
    variables = _variables(4)
    plain = _trainer(variables, images, labels, use_graphs=False)
    fwd = _trainer(variables, images, labels, use_graphs=False, confusion_matrix=np.eye(10))
    try:
        for index in steps[:2]:
            plain.step(LR, index=index)
            fwd.step(LR, index=index)
            assert plain.losses() == fwd.losses()
        for a, b in zip(_slabs(plain), _slabs(fwd)):
            assert (a == b).all()
        rec, post = fwd.recover_labels(images.reshape(N, 28, 28, 1), labels)
        assert (rec == labels).all() and post.shape == (N, 10) and (post[np.arange(N), labels] == 1).all()
        with pytest.raises(RuntimeError):
            plain.recover_labels(images.reshape(N, 28, 28, 1), labels)
    finally:
        plain.close()
        fwd.close()


def test_asset_and_checkpoint_round_trip(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist_classifier import MnistLabelClassifier
    images, labels, steps = _data(5)
    a = _trainer(_variables(5), images, labels, use_graphs=True)
    b = clf = None
    try:
        for index in steps[:3]:
            a.step(LR, index=index)
        path = str(tmp_path / "clf.npz")
        a.save_asset(path)
        z = np.load(path)
        assert sorted(z.files) == sorted(R.NAMES) and all(z[n].shape == R.shapes()[n] and z[n].dtype == np.float32 for n in R.NAMES)
        rs = np.random.RandomState(6)
        x = rs.uniform(0, 1, size=(200, 28, 28, 1))
        y = rs.randint(10, size=200)
        acc, p = a.evaluate(x, y)
        clf = MnistLabelClassifier(path)
        assert clf.n_classes == 10
        q = clf.softmax(x)                                   # the same launches: one batch of 200 on both sides
        assert p.shape == q.shape == (200, 10)
        assert (p.view(np.uint32) == q.view(np.uint32)).all(), float(np.abs(p - q).max())
        # ... and in two batches, the second one short (the GEMMs of another batch size sum in another order: same launches on both sides again)
        assert (a.evaluate(x, y, batch=128)[1].view(np.uint32) == clf.softmax(x, batch=128).view(np.uint32)).all()
        pred = clf.predict(x)
        assert (pred == np.argmax(q, axis=1)).all() and acc == float((pred == y).mean())
        ref = R.softmax(R.forward({n: a.P.get(n) for n in R.NAMES}, x)["logits"])
        print("softmax against float64: max difference %.2e" % np.abs(p - ref).max())
        assert np.abs(p - ref).max() <= 2e-3                 # (the CIFAR evaluator's own bound, tests/test_gpu_label_classifier.py)
        feat = clf.features(x[:7])
        assert feat.shape == (7, 1024) and (feat >= 0).all()
        assert_close(feat, R.forward({n: a.P.get(n) for n in R.NAMES}, x[:7])["feat"], 1e-4, "features")
        clf.close()
        clf = None
        # the checkpoint: a fresh trainer that loads it takes a bit-identical fourth step (weights, Adam slots, step count, dropout stream)
        sd = a.state_dict()
        b = _trainer(_variables(9), images, labels, use_graphs=True)
        b.load_state_dict(sd)
        assert b.steps == 3 and b.rng_offset() == a.rng_offset() == 3 * B * 1024 // 4
        a.step(LR, index=steps[3])
        b.step(LR, index=steps[3])
        for u, v in zip(_slabs(a), _slabs(b)):
            assert (u == v).all()
        assert a.losses() == b.losses()
        # ... and, left to draw for themselves, both draw the same batch next
        a.step(LR)
        b.step(LR)
        assert (_slabs(a)[0] == _slabs(b)[0]).all()
    finally:
        for o in (a, b, clf):
            if o is not None:
                o.close()
