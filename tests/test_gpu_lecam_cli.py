"""train_cifar.py --lecam through the reference-compatible launcher (cifar10/gan_resnet.py): exit status, the log's lecam_a_real /
lecam_a_fake / lecam_reg, the checkpoint's anchors, and a second launch that restores them and goes on.

B = 8; every iteration is five critic steps, five updates of the anchors; the gate opens at the second step, so the R the sample
period logs (the last step's) is positive.  The second launch restores the first one's newest checkpoint: its update count goes on
from the restored one by five per iteration it trains (one logged line each)."""
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
            "--log_file", os.path.join(str(tmp_path), "log_%s_%d.txt" % (expt, niters)), "--parent_dir", str(tmp_path), "--expt_dir", expt,
            "--ngpus", "1", "--multi_gpu_multi_batch", "--niters", str(niters), "--batch_size", str(B), "--synthetic",
            "--synthetic_kind", "templates", "--sample_every", "1", "--inception_freq", "0", "--generated_label_accuracy_freq", "0",
            "--early_checkpoint_every", "1"] + extra


def _values(text, name):
    return [float(v) for v in re.findall(r"%s: ([-0-9.e]+)" % name, text)]


def test_a_short_run_logs_the_anchors_and_a_second_launch_restores_them(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.host import latest_checkpoint, load_checkpoint
    states, updates = [], 0
    for niters in (1, 2):
        argv = _argv(tmp_path, "l1", niters, ["--lecam", "0.3", "--lecam_decay", "0.9"])
        r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        text = open(argv[argv.index("--log_file") + 1]).read()
        assert text.count("lecam = 0.3") == 1, text[:2000]
        a_real, a_fake, reg = (_values(text, k) for k in ("lecam_a_real", "lecam_a_fake", "lecam_reg"))
        assert len(a_real) == len(a_fake) == len(reg) >= 1, text[-3000:]             # one line per iteration trained
        print("niters %d: a_real %r a_fake %r reg %r" % (niters, a_real, a_fake, reg))
        assert np.isfinite(a_real + a_fake + reg).all() and min(reg) > 0 and a_real[-1] != a_fake[-1]
        sd = load_checkpoint(latest_checkpoint(os.path.join(str(tmp_path), "l1", "checkpoint")))
        st = np.asarray(sd["_lecam_state"], np.float32)
        updates += 5 * len(reg)
        assert st.shape == (8,) and st[2] == updates and st[5] == 0, (st, updates)   # the second launch went on from the first one's count
        assert abs(float(st[0]) - a_real[-1]) <= 1e-6 * max(1.0, abs(a_real[-1])) and abs(float(st[1]) - a_fake[-1]) <= 1e-6 * max(1.0, abs(a_fake[-1]))
        assert ("restore model from" in text) == (niters == 2)
        states.append(st)
    assert not np.array_equal(states[0][:2], states[1][:2])


def test_a_bad_decay_is_refused_before_the_run_is_set_up(tmp_path):
    argv = _argv(tmp_path, "l2", 1, ["--lecam", "0.3", "--lecam_decay", "1.0"])
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0
    assert "lecam_decay must lie in [0, 1)" in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert not os.path.exists(os.path.join(str(tmp_path), "l2"))
