"""A training step of the label classifier on the engine against the float64 restatement (tests/classifier_ref.py), its captured
form against its eager form, and the way out: the asset LabelClassifier reads and the checkpoint."""
import numpy as np
import pytest
import torch

from tests import classifier_ref as R
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu
B, N = 16, 64
LR, MOM, WD = 0.1, 0.9, 1e-4


def _data(K, seed=0):
    rs = np.random.RandomState(seed)
    # smooth blobs + noise rather than white noise: keeps the batch statistics away from degenerate values
    base = rs.randint(0, 256, size=(N, 3, 4, 4)).repeat(8, axis=2).repeat(8, axis=3)
    images = np.clip(base + rs.randint(-30, 31, size=(N, 3, 32, 32)), 0, 255).astype(np.uint8).reshape(N, 3072)
    labels = rs.randint(K, size=N).astype(np.int32)
    steps = []
    for _ in range(4):
        index = rs.randint(N, size=B).astype(np.int32)
        sf = np.concatenate([rs.randint(-4, 5, size=(B, 2)), rs.randint(2, size=(B, 1))], axis=1).astype(np.int32)
        sf[0], sf[1] = (4, -4, 1), (-3, 2, 0)
        steps.append((index, sf))
    return images, labels, steps


def _variables(K, seed=0):
    """The trainer's initialisation, jittered so that no gamma / beta / bias gradient is trivially zero.  The batch norms inside the
    blocks get gamma ~ 0.45, beta ~ 1.9: a ReLU network's gradient jumps where a pre-activation crosses zero, so float32 and float64
    legitimately disagree about every element that sits within float32's forward error of zero -- ONE such element moves a whole
    filter-gradient column by ~1e-2 of its scale (measured with PyTorch's own float32 against its float64 on a zero-centred batch:
    worst variable 1e-2 .. 2.6e-2, median 2e-6).  Offsetting the pre-activations makes such elements rare enough that the seeds below
    have none (KINK_MARGIN, checked on the reference in the test); the masked ReLU backward itself is covered by the op tests and by
    tests/test_gpu_classifier_training.py."""
    from rcgan_amd.classifier import create_classifier_variables
    rs = np.random.RandomState(100 + seed)
    out = []
    for n, s, init in create_classifier_variables(seed, K):
        fc = n.startswith("fc|")
        if n.endswith("|gamma"):
            init = ((1.0 if fc else 0.45) * (1.0 + 0.1 * rs.randn(*s))).astype(np.float32)
        elif n.endswith("|beta"):
            init = ((0.0 if fc else 1.9) + (0.1 if fc else 0.03) * rs.randn(*s)).astype(np.float32)
        elif n == "fc|fc_bias":
            init = (0.1 * rs.randn(*s)).astype(np.float32)
        out.append((n, s, init))
    return out


# No pre-activation of the float64 reference may sit closer to a ReLU kink than this in any of the three compared steps: a third to a
# half of the largest float32 forward error of the restatement itself on these batches (1.0e-5 .. 1.6e-5, PyTorch float32 against float64;
# the error at a typical element is an order of magnitude below that largest one).
KINK_MARGIN = 5e-6
SEEDS = {10: 0, 100: 13}      # data / initialisation seeds whose reference batches keep that margin


def _trainer(K, variables, images, labels, use_graphs, arena=2 << 30):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.classifier import LabelClassifierTrainer
    t = LabelClassifierTrainer(K, batch_size=B, momentum=MOM, weight_decay=WD, nesterov=False, pad=4, use_graphs=use_graphs,
                               variables=variables, arena_bytes=arena)
    t.load_data(images, labels)
    return t


def _slabs(t):
    with torch.cuda.stream(t.ctx.stream):
        v, m = t.P.value.cpu().numpy(), t.P.m.cpu().numpy()
    t.ctx.sync()
    return v.view(np.uint32), m.view(np.uint32)


@pytest.mark.parametrize("K", [10, 100])
def test_training_step_against_float64(K):
    images, labels, steps = _data(K, SEEDS[K])
    variables = _variables(K, SEEDS[K])
    t = _trainer(K, variables, images, labels, use_graphs=False)
    try:
        P = {n: torch.from_numpy(np.asarray(i, np.float64)) for n, _, i in variables}
        A = {n: torch.zeros_like(v) for n, v in P.items()}
        before = {n: v.clone() for n, v in P.items()}
        for k, (index, sf) in enumerate(steps[:3]):
            x, y = R.augment(images, labels, index, sf)
            R.TRACE = []
            try:
                loss_ref, acc_ref, G = R.sgd_step(P, A, x, y, LR, MOM, WD, False)
            finally:
                trace, R.TRACE = R.TRACE, None
            nearest = min(float(v.abs().min()) for _, v in trace)
            assert nearest >= KINK_MARGIN, "step %d: a reference pre-activation %.1e from a ReLU kink: the comparison is ill-posed" % (k, nearest)
            t.step(LR, index=index, shift_flip=sf)
            loss, acc = t.losses()
            print("K=%d step %d: loss %.7f (float64 %.7f), batch accuracy %.4f (%.4f)" % (K, k, loss, loss_ref, acc, acc_ref))
            if k == 0:
                assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
                got = t.get_grads()
                assert set(got) == set(G) and len(got) == 95
                worst = max((float(np.abs(got[n] - G[n].numpy()).max() / (np.abs(G[n].numpy()).max() + 1e-12)), n) for n in G)
                print("K=%d: worst gradient error %.3e of its own scale (%s)" % ((K,) + worst))
                for n in G:
                    assert np.abs(G[n].numpy()).max() > 0, n
                    assert_close(got[n], G[n].numpy(), 1e-2, "gradient of " + n)
        worst = (0.0, "")
        for n in P:
            upd_ref = (P[n] - before[n]).numpy()
            upd = t.P.get(n).astype(np.float64) - before[n].numpy()
            worst = max(worst, (float(np.abs(upd - upd_ref).max() / (np.abs(upd_ref).max() + 1e-12)), n))
            assert_close(upd, upd_ref, 1e-2, "update of " + n + " after three steps")
        print("K=%d: worst update error after three steps %.3e of its own scale (%s)" % ((K,) + worst))
    finally:
        t.close()


def test_captured_steps_equal_eager_steps_bit_for_bit():
    K = 20
    images, labels, steps = _data(K, 1)
    variables = _variables(K, 1)
    eager = _trainer(K, variables, images, labels, use_graphs=False)
    graph = _trainer(K, variables, images, labels, use_graphs=True)
    try:
        # the captured trainer rehearses its first step eagerly, captures the second and replays from then on: four steps give three
        # that ran from the graph
        for k, (index, sf) in enumerate(steps):
            eager.step(LR if k < 3 else 0.01, index=index, shift_flip=sf)
            graph.step(LR if k < 3 else 0.01, index=index, shift_flip=sf)
            (ve, me), (vg, mg) = _slabs(eager), _slabs(graph)
            assert (ve == vg).all() and (me == mg).all(), "step %d" % k
            assert eager.losses() == graph.losses()
        assert graph._graph is not None and eager._graph is None
    finally:
        eager.close()
        graph.close()


def test_asset_and_checkpoint_round_trip(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.eval_cifar import LabelClassifier
    K = 20
    images, labels, steps = _data(K, 2)
    a = _trainer(K, _variables(K, 2), images, labels, use_graphs=True, arena=6 << 30)
    b = clf = None
    try:
        for index, sf in steps[:3]:
            a.step(LR, index=index, shift_flip=sf)
        # the asset: what LabelClassifier computes from it is what the trainer's own evaluation computes, bit for bit
        path = str(tmp_path / "clf.npz")
        a.save_asset(path)
        rs = np.random.RandomState(3)
        x = np.clip(rs.randint(0, 256, size=(1000, 4, 4, 3)).repeat(8, axis=1).repeat(8, axis=2) + rs.randint(-30, 31, size=(1000, 32, 32, 3)), 0, 255)
        y = rs.randint(K, size=1000)
        acc, p = a.evaluate(x, y)
        clf = LabelClassifier(0, asset=path)
        assert clf.n_classes == K
        q = clf.softmax(x)
        assert p.shape == q.shape == (1000, K)
        assert (p.view(np.uint32) == q.view(np.uint32)).all(), float(np.abs(p - q).max())
        assert acc == float((np.argmax(q, 1) == y).mean())
        ref = R.softmax({n: torch.from_numpy(a.P.get(n).astype(np.float64)) for n in a.P.names}, x)
        assert np.abs(p - ref).max() <= 2e-3, np.abs(p - ref).max()          # (the evaluator's own bound, test_gpu_label_classifier.py)
        clf.close()
        clf = None
        # the checkpoint: a fresh trainer that loads it takes a bit-identical fourth step
        sd = a.state_dict()
        b = _trainer(K, _variables(K, 5), images, labels, use_graphs=True)
        b.load_state_dict(sd)
        assert b.steps == 3
        index, sf = steps[3]
        a.step(LR, index=index, shift_flip=sf)
        b.step(LR, index=index, shift_flip=sf)
        (va, ma), (vb, mb) = _slabs(a), _slabs(b)
        assert (va == vb).all() and (ma == mb).all()
        # ... and, left to draw for themselves, both draw the same batch next
        a.step(LR)
        b.step(LR)
        assert (_slabs(a)[0] == _slabs(b)[0]).all()
    finally:
        for o in (a, b, clf):
            if o is not None:
                o.close()


def test_standard_initialisation_step_against_float64():
    """The same comparison at the trainer's own initialisation (gamma 1, beta 0 plus jitter), where half of every block's
    pre-activations are masked by the ReLU -- the case the offset batch norms of test_training_step_against_float64 leave to the op
    tests.  Here a handful of the 4.8 million pre-activations sit within float32's forward error of zero, and each one that float32
    masks differently moves one gradient column (and, diluted, the layers below it) by ~1e-2 of its scale in ANY float32
    implementation, so a per-variable maximum cannot be asserted.  What can be: the loss (no kink in its value) at the issue's bound,
    and the MEDIAN over the 95 variables of that per-variable maximum error at the same 1e-2 -- a wrong ReLU mask in the backward
    pass puts an error of order one into every variable below it, a flipped element reaches a few columns."""
    K = 10
    images, labels, steps = _data(K, 0)
    from rcgan_amd.classifier import create_classifier_variables
    rs = np.random.RandomState(100)
    variables = []
    for n, s, init in create_classifier_variables(0, K):
        if n.endswith("|gamma"):
            init = (1.0 + 0.1 * rs.randn(*s)).astype(np.float32)
        elif n.endswith("|beta") or n == "fc|fc_bias":
            init = (0.1 * rs.randn(*s)).astype(np.float32)
        variables.append((n, s, init))
    t = _trainer(K, variables, images, labels, use_graphs=False)
    try:
        index, sf = steps[0]
        x, y = R.augment(images, labels, index, sf)
        loss_ref, _, G = R.loss_and_grads({n: torch.from_numpy(np.asarray(i, np.float64)) for n, _, i in variables}, x, y)
        t.step(LR, index=index, shift_flip=sf)
        loss, _ = t.losses()
        got = t.get_grads()
        errs = sorted(float(np.abs(got[n] - G[n].numpy()).max() / (np.abs(G[n].numpy()).max() + 1e-12)) for n in G)
        print("standard initialisation: loss %.7f (float64 %.7f); per-variable max error: median %.3e, worst %.3e"
              % (loss, loss_ref, errs[len(errs) // 2], errs[-1]))
        assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
        assert all(np.isfinite(got[n]).all() for n in got)
        assert errs[len(errs) // 2] <= 1e-2, errs[len(errs) // 2]
    finally:
        t.close()


def test_high_f32_matmul_precision_steps():
    """--f32_matmul_precision high (split-bf16 matrix cores) through the trainer: eager and replayed steps are the same bits (the
    captured graph keeps the setting), the setting is not ignored, and the losses stay within the project's bound between the two
    precisions (1e-3 relative, tests/test_gpu_f32_precision.py)."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.classifier import LabelClassifierTrainer
    K = 20
    images, labels, steps = _data(K, 3)
    variables = _variables(K, 3)

    def make(precision, use_graphs):
        t = LabelClassifierTrainer(K, batch_size=B, momentum=MOM, weight_decay=WD, pad=4, use_graphs=use_graphs, variables=variables,
                                   arena_bytes=2 << 30, f32_matmul_precision=precision)
        t.load_data(images, labels)
        return t
    ts = dict(highest=make("highest", True), high=make("high", True), high_eager=make("high", False))
    try:
        for k, (index, sf) in enumerate(steps[:3]):          # the graph trainers: eager rehearsal, capture + launch, replay
            for t in ts.values():
                t.step(LR, index=index, shift_flip=sf)
            lo = {name: t.losses()[0] for name, t in ts.items()}
            print("step %d losses: %s" % (k, lo))
            assert lo["high"] == lo["high_eager"]
            assert abs(lo["high"] - lo["highest"]) <= 1e-3 * max(abs(lo["highest"]), 1e-3), lo
            assert (_slabs(ts["high"])[0] == _slabs(ts["high_eager"])[0]).all(), k
        assert ts["high"]._graph is not None
        assert not (_slabs(ts["high"])[0] == _slabs(ts["highest"])[0]).all()
        acc, p = ts["high"].evaluate(np.zeros((8, 32, 32, 3)) + np.arange(8).reshape(8, 1, 1, 1) * 30.0, np.zeros(8, int), batch=8)
        assert p.shape == (8, K) and np.isfinite(p).all() and np.allclose(p.sum(1), 1.0, atol=1e-5)
    finally:
        for t in ts.values():
            t.close()
