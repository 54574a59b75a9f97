"""train_cifar.py --diversity through the reference-compatible launcher (cifar10/gan_resnet.py): exit status, the log's option line and
its diversity_ratio / diversity_clamped / diversity_masked; a negative weight fails before the GPU is touched.

B = 8, three iterations: iteration 0 has no generator step, so the sample period logs the term from iteration 1 on.  The generator
labels go through pair_generator_labels, so no pair is masked."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8


def _argv(tmp_path, expt, niters, extra):
    return [sys.executable, os.path.join(ROOT, "cifar10", "gan_resnet.py"), "--algorithm", "rcgan", "--alpha", "0.6",
            "--log_file", os.path.join(str(tmp_path), "log_%s.txt" % expt), "--parent_dir", str(tmp_path), "--expt_dir", expt,
            "--ngpus", "1", "--multi_gpu_multi_batch", "--niters", str(niters), "--batch_size", str(B), "--synthetic",
            "--synthetic_kind", "templates", "--sample_every", "1", "--inception_freq", "0", "--generated_label_accuracy_freq", "0",
            "--early_checkpoint_every", "1"] + extra


def _values(text, name):
    return [float(v) for v in re.findall(r"%s: ([-0-9.e]+)" % name, text)]


def test_a_short_run_logs_the_term(tmp_path):
    argv = _argv(tmp_path, "d1", 3, ["--diversity", "1", "--diversity_tau", "0.8"])
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = open(argv[argv.index("--log_file") + 1]).read()
    assert text.count("diversity = 1.0 (tau 0.8)") == 1, text[:2000]
    ratio, clamped, masked = (_values(text, k) for k in ("diversity_ratio", "diversity_clamped", "diversity_masked"))
    print("ratio %r clamped %r masked %r" % (ratio, clamped, masked))
    assert len(ratio) == len(clamped) == len(masked) == 2, text[-3000:]          # iterations 1 and 2
    assert masked == [0.0, 0.0]
    assert np.isfinite(ratio).all() and min(ratio) > 0
    assert all(0.0 <= c <= 1.0 for c in clamped)


def test_a_negative_weight_is_refused_before_the_run_is_set_up(tmp_path):
    argv = _argv(tmp_path, "d2", 1, ["--diversity", "-1"])
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0
    assert "diversity must be finite and >= 0" in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert not os.path.exists(os.path.join(str(tmp_path), "d2"))
