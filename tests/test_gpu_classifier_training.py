"""The label classifier learns on the engine, and the asset it writes is what the GAN trainer's --label_classifier scores with."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = os.path.join(ROOT, "profiles", "classifier_templates_reference.json")
K, N_TRAIN, BATCH = 20, 12800, 128


def test_it_learns_the_class_patterns():
    """250 steps on synthetic_cifar(12800, 1234, "templates", 20) in consecutive batches of 128 (lr 0.1, momentum 0.9, weight decay 1e-4,
    no Nesterov, no augmentation); held out synthetic_cifar(1000, 1235, "templates", 20) scored as ONE batch.  The engine may end no more
    than 0.05 below the LOWEST of the three seeds of the float32 PyTorch-CPU restatement (scripts/classifier_reference_curve.py ->
    profiles/classifier_templates_reference.json): 1000 held-out images at accuracy ~0.95 have a binomial standard error of 0.007 and
    another initialisation stream moves the curve by a few hundredths more; a broken gradient (chance 0.05, or a stall near 0.5) cannot
    meet it."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from rcgan_amd.classifier import LabelClassifierTrainer
    ref = json.load(open(CURVE))
    steps = ref["steps"]
    assert ref["n_classes"] == K and ref["batch"] == BATCH and len(ref["seeds"]) == 3 and steps % 50 == 0
    finals = [c[str(steps)] for c in ref["seeds"].values()]
    assert max(finals) - min(finals) <= 0.05, finals          # else the recorded run has to be lengthened, not the margin widened
    tx, ty = D.synthetic_cifar(N_TRAIN, 1234, "templates", K)
    vx, vy = D.synthetic_cifar(1000, 1235, "templates", K)
    held = vx.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    t = LabelClassifierTrainer(K, batch_size=BATCH, momentum=0.9, weight_decay=1e-4, nesterov=False, pad=0, seed=0)
    try:
        t.load_data(tx, ty)
        still = np.zeros((BATCH, 3), np.int32)
        curve = {}
        for step in range(1, steps + 1):
            lo = ((step - 1) * BATCH) % N_TRAIN
            t.step(0.1, index=np.arange(lo, lo + BATCH), shift_flip=still)
            if step % 50 == 0:
                curve[step] = t.evaluate(held, vy)[0]
        print("engine held-out accuracy %s; reference seeds at step %d: %s" % (curve, steps, finals))
        assert curve[steps] >= min(finals) - 0.05, (curve, finals)
    finally:
        t.close()


def _run(module, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_both_command_lines_end_to_end(tmp_path):
    asset = str(tmp_path / "clf20.npz")
    data_flags = ["--dataset", "cifar100", "--coarse_labels", "--synthetic", "--synthetic_kind", "templates"]
    _run("rcgan_amd.train_classifier", data_flags + ["--synthetic_samples", str(N_TRAIN), "--no_augment", "--max_steps", "250", "--out", asset,
                                                     "--log_file", str(tmp_path / "clf_log.txt")])
    z = np.load(asset)
    assert z["fc|fc_weights"].shape == (64, K) and sum(1 for k in z.files if z[k].dtype.kind == "f" and z[k].ndim > 0) == 95
    clf_log = open(str(tmp_path / "clf_log.txt")).read()
    held = [float(v) for v in re.findall(r"held-out accuracy ([0-9.]+) \(", clf_log)]
    print("train_classifier: held-out accuracy per epoch %s" % held)
    assert held and all(0.0 <= v <= 1.0 for v in held), clf_log[-2000:]
    log = str(tmp_path / "gan_log.txt")
    _run("rcgan_amd.train_cifar", data_flags + ["--niters", "20", "--batch_size", "16", "--generated_label_accuracy_freq", "10",
                                                "--label_classifier", asset, "--ngpus", "1", "--log_file", log, "--parent_dir", str(tmp_path), "--expt_dir", "run",
                                                "--inception_freq", "0", "--sample_freq", "1000000"])
    text = open(log).read()
    vals = [float(v) for v in re.findall(r"generated label accuracy: ([0-9.eE+-]+)", text)]
    print("train_cifar --label_classifier: generated label accuracy %s" % vals)
    assert len(vals) == 3, text[-2000:]                      # iterations 10 and 20, plus the final one
    assert all(0.0 <= v <= 1.0 for v in vals), vals
    assert "skipped" not in text
