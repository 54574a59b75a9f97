"""The MNIST label classifier learns on the engine, and the asset it writes is what train_mnist.py --label_classifier scores with."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = os.path.join(ROOT, "profiles", "mnist_classifier_templates_reference.json")
N_TRAIN, BATCH = 6400, 128


def test_it_learns_the_class_patterns():
    """100 steps of Adam (lr 1e-3, keep_prob 0.5) on data_mnist.synthetic(6400, 1234, "templates") in consecutive batches of 128;
    held out synthetic(1000, 1235, "templates"), no dropout.  The three seeds of the float32 PyTorch-CPU restatement
    (scripts/mnist_classifier_reference_curve.py -> profiles/mnist_classifier_templates_reference.json) end at 1.000, 0.999 and 1.000:
    within 0.05 of each other and above 0.9, as the recorded run has to be.  The engine may end no more than 0.05 below the LOWEST of
    them: 1000 held-out images have a binomial standard error of at most 0.007 there and another initialisation / mask stream moves
    the curve by a few hundredths more; chance (0.1) or a stall cannot meet it."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data_mnist as DM
    from rcgan_amd.mnist_classifier import MnistClassifierTrainer
    ref = json.load(open(CURVE))
    steps, lr = ref["steps"], ref["lr"]
    assert ref["batch"] == BATCH and ref["train"][0] == N_TRAIN and ref["keep_prob"] == 0.5 and len(ref["seeds"]) == 3 and steps <= 300
    finals = [c[str(steps)] for c in ref["seeds"].values()]
    assert max(finals) - min(finals) <= 0.05, finals          # else the recorded run has to be lengthened, not the margin widened
    assert min(finals) >= 0.9, finals
    tx, ty = DM.synthetic(N_TRAIN, 1234, "templates")
    vx, vy = DM.synthetic(1000, 1235, "templates")
    t = MnistClassifierTrainer(batch_size=BATCH, keep_prob=ref["keep_prob"], seed=0)
    try:
        t.load_data(tx, ty)                                   # raw pixel values: divided by 255 on the way in
        curve = {}
        for step in range(1, steps + 1):
            lo = ((step - 1) * BATCH) % N_TRAIN
            t.step(lr, index=np.arange(lo, lo + BATCH))
            if step % 50 == 0 or step == steps:
                curve[step] = t.evaluate(vx / 255., vy)[0]
        print("engine held-out accuracy %s; reference seeds at step %d: %s" % (curve, steps, finals))
        assert curve[steps] >= min(finals) - 0.05, (curve, finals)
    finally:
        t.close()


def _run(module, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_both_command_lines_end_to_end(tmp_path):
    ref = json.load(open(CURVE))
    asset = str(tmp_path / "mnist_clf.npz")
    _run("rcgan_amd.train_mnist_classifier", ["--synthetic", "--synthetic_kind", "templates", "--synthetic_samples", str(N_TRAIN),
                                              "--max_steps", str(ref["steps"]), "--lr", str(ref["lr"]), "--out", asset,
                                              "--log_file", str(tmp_path / "clf_log.txt")])
    z = np.load(asset)
    shapes = {"conv1|w": (5, 5, 1, 32), "conv1|b": (32,), "conv2|w": (5, 5, 32, 64), "conv2|b": (64,), "fc1|w": (3136, 1024),
              "fc1|b": (1024,), "fc2|w": (1024, 10), "fc2|b": (10,)}
    assert {k: z[k].shape for k in z.files} == shapes
    clf_log = open(str(tmp_path / "clf_log.txt")).read()
    held = [float(v) for v in re.findall(r"epoch \d+ step \d+ .* held-out accuracy ([0-9.]+) \(", clf_log)]
    print("train_mnist_classifier: held-out accuracy per epoch %s" % held)
    assert len(held) == ref["steps"] // (N_TRAIN // BATCH) and all(0.0 <= v <= 1.0 for v in held), clf_log[-2000:]
    out = _run("rcgan_amd.train_mnist", ["--train", "--synthetic", "--synthetic_kind", "templates", "--synthetic_size", "500", "--batch_size", "100",
                                         "--epoch", "2", "--sample_epochs", "1", "--label_classifier", asset,
                                         "--checkpoint_dir", str(tmp_path), "--checkpoint", "run", "--recover_epoch", "0"])
    vals = [float(v) for v in re.findall(r"mean generated label accuracy=([0-9.eE+-]+)", out)]
    print("train_mnist --label_classifier: generated label accuracy %s" % vals)
    assert len(vals) == 2, out[-2000:]                       # every sampling epoch
    assert all(0.0 <= v <= 1.0 for v in vals), vals
    assert "skipped" not in out
