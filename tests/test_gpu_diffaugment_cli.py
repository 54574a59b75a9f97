"""train_cifar.py --diffaugment through the reference-compatible launcher (cifar10/gan_resnet.py): exit status and log."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(tmp_path, policy):
    log = os.path.join(str(tmp_path), "log.txt")
    argv = [sys.executable, os.path.join(ROOT, "cifar10", "gan_resnet.py"), "--algorithm", "rcgan", "--alpha", "0.6", "--log_file", log,
            "--parent_dir", str(tmp_path), "--expt_dir", "a1", "--ngpus", "1", "--multi_gpu_multi_batch", "--niters", "3", "--batch_size", "8",
            "--synthetic", "--synthetic_kind", "templates", "--sample_freq", "0", "--inception_freq", "0",
            "--generated_label_accuracy_freq", "100", "--early_checkpoint_every", "4", "--diffaugment", policy]
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r, (open(log).read() if os.path.exists(log) else "")


def test_a_short_run_with_the_option_exits_cleanly_and_logs_the_policy(tmp_path):
    r, log = _launch(tmp_path, "translation,cutout")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert log.count("diffaugment = translation,cutout") == 1, log[:2000]
    assert "generated label accuracy: " in log, log[-2000:]          # the run got to its final evaluation


def test_an_unknown_policy_name_is_refused_with_the_allowed_values(tmp_path):
    r, log = _launch(tmp_path, "blur")
    assert r.returncode != 0
    err = r.stderr.decode()
    assert "Unknown diffaugment policy 'blur'" in err and "color,translation,cutout" in err, err[-2000:]
    assert "diffaugment" not in log          # refused before the run is set up
