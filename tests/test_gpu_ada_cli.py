"""train_cifar.py --ada_target through the reference-compatible launcher (cifar10/gan_resnet.py): exit status, the log's ada_p / ada_r,
and the checkpoint's controller state.

B = 8 and --ada_interval 2: p moves by B * interval / ada_images per update, so --ada_images 64 makes one update a quarter of the
range.  The run is ONE iteration: five critic steps, two updates.  On the class-pattern images the critic has every real score
above zero by its third step (measured: r = 0.5 at the first update, 1.0 at the second, at the default learning rate), so p has left
0 when the iteration ends and the sample period logs it; a few iterations later the young generator drags the real scores below
zero again and p is back at 0, which is why the run stops here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, INTERVAL = 8, 2
IMAGES = 4 * B * INTERVAL             # four updates in one direction cross the whole range


def test_a_short_run_logs_p_and_r_and_its_checkpoint_restores_p(tmp_path):
    log = os.path.join(str(tmp_path), "log.txt")
    argv = [sys.executable, os.path.join(ROOT, "cifar10", "gan_resnet.py"), "--algorithm", "rcgan", "--alpha", "0.6", "--log_file", log,
            "--parent_dir", str(tmp_path), "--expt_dir", "a1", "--ngpus", "1", "--multi_gpu_multi_batch", "--niters", "1", "--batch_size", str(B),
            "--synthetic", "--synthetic_kind", "templates", "--sample_every", "1", "--inception_freq", "0",
            "--generated_label_accuracy_freq", "0", "--early_checkpoint_every", "4",
            "--diffaugment", "color,translation,cutout", "--ada_target", "0.6", "--ada_interval", str(INTERVAL), "--ada_images", str(IMAGES)]
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = open(log).read()
    assert text.count("ada_target = 0.6") == 1, text[:2000]
    p = re.findall(r"ada_p: ([-0-9.e]+)", text)
    rr = re.findall(r"ada_r: ([-0-9.e]+)", text)
    assert len(p) == 1 and len(rr) == 1, text[-3000:]
    p, rr = float(p[0]), float(rr[0])
    print("ada_p %r ada_r %r" % (p, rr))
    assert 0.0 < p <= 1.0 and p * IMAGES / (B * INTERVAL) == round(p * IMAGES / (B * INTERVAL)), "p is a whole number of steps away from 0"
    assert -1.0 <= rr <= 1.0
    # the checkpoint carries the controller, and a fresh engine restored from it reports the logged p
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    from rcgan_amd.host import latest_checkpoint, load_checkpoint
    sd = load_checkpoint(latest_checkpoint(os.path.join(str(tmp_path), "a1", "checkpoint")))
    st = np.asarray(sd["_ada_state"], np.float32)
    assert st.shape == (8,) and float(st[0]) == p and float(st[4]) == rr and st[5] == 5 // INTERVAL and st[3] == 1
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", diffaugment="color,translation,cutout",
                   ada_target=0.6, ada_interval=INTERVAL, ada_images=IMAGES, arena_bytes=1 << 30)
    try:
        assert m.ada_report() == dict(p=0.0, r_last=0.0, updates=0)
        m.load_state_dict(sd)
        assert m.ada_report() == dict(p=p, r_last=rr, updates=2)
    finally:
        m.ctx.close()


def test_the_option_without_a_policy_is_refused_before_the_run_is_set_up(tmp_path):
    log = os.path.join(str(tmp_path), "log.txt")
    argv = [sys.executable, os.path.join(ROOT, "cifar10", "gan_resnet.py"), "--algorithm", "rcgan", "--log_file", log,
            "--parent_dir", str(tmp_path), "--expt_dir", "a2", "--niters", "1", "--batch_size", str(B), "--synthetic", "--ada_target", "0.6"]
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0
    assert "needs a non-empty diffaugment policy" in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert not os.path.exists(os.path.join(str(tmp_path), "a2"))
