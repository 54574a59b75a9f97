"""The label classifier trained on NOISY labels with the forward-corrected loss: a training step against the float64 restatement
(tests/classifier_ref.py + tests/forward_xent_ref.py), its captured form against its eager form with the confusion matrix replaced
between two launches, learning and label recovery under 40 % label noise against the recorded PyTorch-CPU reference, and the command
line end to end."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import classifier_ref as R
from tests import forward_xent_ref as FR
from tests import test_gpu_classifier_step as S
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.path.join(ROOT, "profiles", "classifier_forward_reference.json")
LR, MOM, WD = S.LR, S.MOM, S.WD
K_TRAIN, N_TRAIN, BATCH = 20, 12800, 128


def _dense_C(K, seed):
    """A dense random confusion matrix, diagonal-heavy, as the device holds it: float32 values (rows sum to 1 within float32 rounding)."""
    rs = np.random.RandomState(500 + seed)
    Cm = 0.5 * np.eye(K) + 0.5 * rs.dirichlet(np.ones(K), size=K)
    return Cm.astype(np.float32).astype(np.float64)


def _trainer(K, variables, images, labels, use_graphs, Cm):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.classifier import LabelClassifierTrainer
    t = LabelClassifierTrainer(K, batch_size=S.B, momentum=MOM, weight_decay=WD, nesterov=False, pad=4, use_graphs=use_graphs,
                               variables=variables, arena_bytes=2 << 30, confusion_matrix=Cm)
    t.load_data(images, labels)
    return t


# data / initialisation seed of test_gpu_classifier_step._data / _variables whose float64 reference batches keep its KINK_MARGIN under THIS
# loss in all three steps (nearest pre-activation 2.1e-5; seeds 0 and 1 come within 5e-7 and 4.9e-6 of a kink)
STEP_SEED = 2


def test_forward_training_step_against_float64():
    """Three steps, K = 10, a dense random C, the batch and the offset pre-activations of test_training_step_against_float64 and its
    tolerances: loss 2e-5, gradients and three-step updates 1e-2 of each variable's scale."""
    K = 10
    images, labels, steps = S._data(K, STEP_SEED)
    variables = S._variables(K, STEP_SEED)
    Cm = _dense_C(K, STEP_SEED)
    t = _trainer(K, variables, images, labels, False, Cm)
    try:
        P = {n: torch.from_numpy(np.asarray(i, np.float64)) for n, _, i in variables}
        A = {n: torch.zeros_like(v) for n, v in P.items()}
        before = {n: v.clone() for n, v in P.items()}
        for k, (index, sf) in enumerate(steps[:3]):
            x, y = R.augment(images, labels, index, sf)
            R.TRACE = []
            try:
                loss_ref, acc_ref, G = FR.sgd_step(P, A, x, y, Cm, LR, MOM, WD, False)
            finally:
                trace, R.TRACE = R.TRACE, None
            nearest = min(float(v.abs().min()) for _, v in trace)
            assert nearest >= S.KINK_MARGIN, "step %d: a reference pre-activation %.1e from a ReLU kink: the comparison is ill-posed" % (k, nearest)
            t.step(LR, index=index, shift_flip=sf)
            loss, acc = t.losses()
            print("forward loss step %d: loss %.7f (float64 %.7f), batch accuracy %.4f (%.4f)" % (k, loss, loss_ref, acc, acc_ref))
            if k == 0:
                assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
                got = t.get_grads()
                assert set(got) == set(G) and len(got) == 95
                worst = max((float(np.abs(got[n] - G[n].numpy()).max() / (np.abs(G[n].numpy()).max() + 1e-12)), n) for n in G)
                print("forward loss: worst gradient error %.3e of its own scale (%s)" % worst)
                for n in G:
                    assert np.abs(G[n].numpy()).max() > 0, n
                    assert_close(got[n], G[n].numpy(), 1e-2, "gradient of " + n)
        worst = (0.0, "")
        for n in P:
            upd_ref = (P[n] - before[n]).numpy()
            upd = t.P.get(n).astype(np.float64) - before[n].numpy()
            worst = max(worst, (float(np.abs(upd - upd_ref).max() / (np.abs(upd_ref).max() + 1e-12)), n))
            assert_close(upd, upd_ref, 1e-2, "update of " + n + " after three steps")
        print("forward loss: worst update error after three steps %.3e of its own scale (%s)" % worst)
    finally:
        t.close()


def test_captured_forward_steps_equal_eager_and_follow_a_new_matrix():
    """Captured steps are the eager steps bit for bit with the forward term.  set_confusion_matrix between two launches of the graph
    takes effect without a recapture: the graph trainer stays equal to the eager one that got the same new matrix, and both part from
    an eager trainer that kept the old one."""
    K = 20
    images, labels, steps = S._data(K, 1)
    variables = S._variables(K, 1)
    C1, C2 = _dense_C(K, 1), _dense_C(K, 2)
    eager = _trainer(K, variables, images, labels, False, C1)
    graph = _trainer(K, variables, images, labels, True, C1)
    stale = _trainer(K, variables, images, labels, False, C1)
    try:
        for k, (index, sf) in enumerate(steps):
            if k == 3:
                gid = graph._graph                 # captured at step 1, replayed at step 2
                assert gid is not None
                eager.set_confusion_matrix(C2)
                graph.set_confusion_matrix(C2)
            for t in (eager, graph, stale):
                t.step(LR, index=index, shift_flip=sf)
            (ve, me), (vg, mg), (vs, ms) = S._slabs(eager), S._slabs(graph), S._slabs(stale)
            assert (ve == vg).all() and (me == mg).all(), "step %d" % k
            assert eager.losses() == graph.losses()
            if k < 3:
                assert (ve == vs).all() and eager.losses() == stale.losses()
            else:
                assert graph._graph == gid and eager._graph is None
                assert eager.losses()[0] != stale.losses()[0] and not (ve == vs).all()
        assert (graph.ctx.download(graph.ct) == C2.T.astype(np.float32)).all()
        with pytest.raises(ValueError):
            graph.set_confusion_matrix(2 * C2)
        with pytest.raises(ValueError):
            graph.set_confusion_matrix(C2[:5, :5])
    finally:
        for t in (eager, graph, stale):
            t.close()


def test_a_trainer_without_a_matrix_has_no_recovery():
    import rcgan_amd  # noqa: F401
    K = 10
    images, labels, _ = S._data(K, 0)
    t = S._trainer(K, S._variables(K, 0), images, labels, use_graphs=False)
    try:
        assert t.ct is None
        with pytest.raises(RuntimeError):
            t.recover_labels(np.zeros((4, 32, 32, 3)), np.zeros(4, int))
        with pytest.raises(RuntimeError):
            t.set_confusion_matrix(np.eye(K))
    finally:
        t.close()


def test_it_learns_and_recovers_labels_under_noise():
    """synthetic_cifar(12800, 1234, "templates", 20) with its labels corrupted once at alpha = 0.6, consecutive batches of 128 (lr 0.1,
    momentum 0.9, weight decay 1e-4, no augmentation), forward loss with the known matrix.  Two numbers at the recorded step count:
    accuracy against the CLEAN labels of held-out synthetic_cifar(1000, 1235, ...) scored as one batch, and label-recovery accuracy on
    the first 2000 training images.  The engine may end at most 0.05 below the LOWEST of the three seeds of the float32 PyTorch-CPU
    restatement on each (scripts/classifier_forward_reference_curve.py -> profiles/classifier_forward_reference.json): the margin and
    the reasoning of test_it_learns_the_class_patterns -- 1000 / 2000 samples at accuracy ~0.9 have a binomial standard error below
    0.01 and another initialisation stream moves the curve by a few hundredths more; a classifier that fitted the noise, or did not
    use the matrix, cannot meet it (the noisy labels agree with the clean ones on 0.60 of the images).  Recorded: held-out 0.894,
    0.877, 0.889; recovery 0.9305, 0.9105, 0.910 at 250 steps."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from rcgan_amd.classifier import LabelClassifierTrainer
    ref = json.load(open(REFERENCE))
    steps, n_rec = ref["steps"], ref["n_recover"]
    assert ref["n_classes"] == K_TRAIN and ref["batch"] == BATCH and ref["alpha"] == 0.6 and n_rec == 2000 and steps % 50 == 0
    held_ref = [c[str(steps)] for c in ref["held_out_accuracy"].values()]
    rec_ref = [c[str(steps)] for c in ref["recovery_accuracy"].values()]
    assert len(held_ref) == 3 and len(rec_ref) == 3
    # else the recorded run has to be lengthened, not the margin widened
    assert max(held_ref) - min(held_ref) <= 0.05, held_ref
    assert max(rec_ref) - min(rec_ref) <= 0.05, rec_ref
    tx, ty = D.synthetic_cifar(N_TRAIN, 1234, "templates", K_TRAIN)
    vx, vy = D.synthetic_cifar(1000, 1235, "templates", K_TRAIN)
    Cm = D.C_ALPHA(ref["alpha"], K_TRAIN)
    noisy = D.noisy_labels(ty, Cm, np.random.RandomState(ref["label_seed"]))
    assert float((noisy == ty).mean()) == ref["noisy_agreement"]
    held = vx.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    first = tx[:n_rec].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    t = LabelClassifierTrainer(K_TRAIN, batch_size=BATCH, momentum=0.9, weight_decay=1e-4, nesterov=False, pad=0, seed=0, confusion_matrix=Cm)
    try:
        t.load_data(tx, noisy)
        still = np.zeros((BATCH, 3), np.int32)
        for step in range(1, steps + 1):
            lo = ((step - 1) * BATCH) % N_TRAIN
            t.step(0.1, index=np.arange(lo, lo + BATCH), shift_flip=still)
        held_acc = t.evaluate(held, vy)[0]
        rec, post = t.recover_labels(first, noisy[:n_rec])
        rec_acc = float((rec == ty[:n_rec]).mean())
        print("engine after %d steps: held-out accuracy %.4f (reference seeds %s), label-recovery accuracy %.4f (reference seeds %s; the noisy "
              "labels agree on %.4f)" % (steps, held_acc, held_ref, rec_acc, rec_ref, float((noisy[:n_rec] == ty[:n_rec]).mean())))
        assert rec.shape == (n_rec,) and post.shape == (n_rec, K_TRAIN) and np.abs(post.sum(axis=1) - 1.0).max() <= 1e-5
        assert (rec == np.argmax(post, axis=1)).all()
        assert held_acc >= min(held_ref) - 0.05, (held_acc, held_ref)
        assert rec_acc >= min(rec_ref) - 0.05, (rec_acc, rec_ref)
    finally:
        t.close()


def test_command_line_end_to_end(tmp_path):
    asset, rec_path, log = str(tmp_path / "clf20.npz"), str(tmp_path / "recovered.npz"), str(tmp_path / "clf_log.txt")
    args = ["--synthetic", "--synthetic_kind", "templates", "--dataset", "cifar100", "--coarse_labels", "--alpha", "0.6", "--loss", "forward",
            "--confusion_matrix", "known", "--recover_out", rec_path, "--max_steps", "250", "--no_augment",
            "--synthetic_samples", str(N_TRAIN), "--out", asset, "--log_file", log]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rcgan_amd.train_classifier"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(asset)
    assert z["fc|fc_weights"].shape == (64, K_TRAIN) and sum(1 for k in z.files if z[k].dtype.kind == "f" and z[k].ndim > 0) == 95
    rz = np.load(rec_path)
    assert set(rz.files) == {"y_noisy", "y_recover", "posterior", "confusion_matrix", "recovery_accuracy", "noisy_agreement"}
    assert rz["y_noisy"].shape == rz["y_recover"].shape == (N_TRAIN,) and rz["posterior"].shape == (N_TRAIN, K_TRAIN)
    assert np.abs(rz["posterior"].sum(axis=1) - 1.0).max() <= 1e-5
    assert (rz["y_recover"] == np.argmax(rz["posterior"], axis=1)).all()
    from rcgan_amd import data as D
    assert (rz["confusion_matrix"] == D.C_ALPHA(0.6, K_TRAIN)).all()
    _, clean = D.synthetic_cifar(N_TRAIN, 1234, "templates", K_TRAIN)
    assert float(rz["recovery_accuracy"]) == float((rz["y_recover"] == clean).mean())
    assert float(rz["noisy_agreement"]) == float((rz["y_noisy"] == clean).mean()) and abs(float(rz["noisy_agreement"]) - 0.6) < 0.02
    text = open(log).read()
    m = re.search(r"label recovery accuracy ([0-9.]+) \(noisy labels agree with clean: ([0-9.]+)\)", text)
    assert m, text[-2000:]
    print("train_classifier --loss forward: recovery accuracy %s, noisy agreement %s" % m.groups())
    assert abs(float(m.group(1)) - float(rz["recovery_accuracy"])) < 1e-4 and abs(float(m.group(2)) - float(rz["noisy_agreement"])) < 1e-4
    assert re.findall(r"held-out accuracy ([0-9.]+) \(", text)


def test_command_line_with_an_estimated_matrix(tmp_path):
    """--confusion_matrix estimate on a small set: a plain cross-entropy stage, the anchor estimate from its soft-max over the training
    set, then the forward-corrected run from a fresh initialisation.  Too short to say anything about the estimate's quality: what is
    checked is that the two stages run, that the matrix handed to the trainer is a valid one and that it is the one written out."""
    asset, rec_path, log = str(tmp_path / "clf.npz"), str(tmp_path / "recovered.npz"), str(tmp_path / "log.txt")
    n = 2560
    args = ["--synthetic", "--synthetic_kind", "templates", "--dataset", "cifar", "--alpha", "0.6", "--label_seed", "3", "--loss", "forward",
            "--confusion_matrix", "estimate", "--estimate_steps", "30", "--anchor_quantile", "0.9", "--recover_out", rec_path,
            "--max_steps", "20", "--no_augment", "--synthetic_samples", str(n), "--out", asset, "--log_file", log]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rcgan_amd.train_classifier"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rz = np.load(rec_path)
    Cm = rz["confusion_matrix"]
    assert Cm.shape == (10, 10) and Cm.min() > 0 and np.abs(Cm.sum(axis=1) - 1.0).max() <= 1e-6
    assert rz["posterior"].shape == (n, 10) and np.abs(rz["posterior"].sum(axis=1) - 1.0).max() <= 1e-5
    text = open(log).read()
    assert "30 steps of plain cross-entropy" in text and "estimated confusion matrix (quantile 0.9)" in text
    assert len(re.findall(r"step 30 lr", text)) == 1 and len(re.findall(r"step 20 lr", text)) >= 1          # stage one, then stage two
    assert re.search(r"label recovery accuracy ([0-9.]+) \(noisy labels agree with clean: ([0-9.]+)\)", text)
    assert np.load(asset)["fc|fc_weights"].shape == (64, 10)
