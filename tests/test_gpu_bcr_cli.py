"""train_cifar.py --bcr_real / --bcr_fake through the reference-compatible launcher (cifar10/gan_resnet.py): exit status, the log's
bcr_real / bcr_fake (one line per iteration trained, finite, non-negative), a checkpoint without any state of the term, which an engine
restores and trains on.  B = 8, the draws on the device, the five critic steps of an iteration as one captured graph."""
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


def test_a_short_run_logs_the_two_means_and_its_checkpoint_restores(tmp_path):
    """ONE training launch of one iteration; its checkpoint is then restored into an engine in this process (the launcher's restore is
    load_state_dict of that file), which trains a critic step on it."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    from rcgan_amd.host import latest_checkpoint, load_checkpoint
    argv = _argv(tmp_path, "b1", 1, ["--bcr_real", "10", "--bcr_fake", "10"])
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = open(argv[argv.index("--log_file") + 1]).read()
    assert text.count("bcr = real 10.0 fake 10.0 (translation)") == 1, text[:2000]
    real, fake = _values(text, "bcr_real"), _values(text, "bcr_fake")
    assert len(real) == len(fake) == 1, text[-3000:]                  # one line per iteration trained
    print("bcr_real %r bcr_fake %r" % (real, fake))
    assert np.isfinite(real + fake).all() and min(real + fake) >= 0 and max(real + fake) > 0
    sd = load_checkpoint(latest_checkpoint(os.path.join(str(tmp_path), "b1", "checkpoint")))
    assert not [k for k in sd if "bcr" in k], "the term has no state"
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=9, use_graphs=False, arena_bytes=2 << 30,
                   bcr_real=10.0, bcr_fake=10.0)
    try:
        m.load_state_dict(sd)
        restored = [k for k in m.get_params() if k in sd]
        assert restored, sorted(sd)[:20]
        for k, v in m.get_params().items():
            if k in sd:
                assert np.array_equal(v, np.asarray(sd[k], np.float32).reshape(v.shape)), k
        rs = np.random.RandomState(0)
        lab = rs.randint(10, size=B)
        m.set_inputs(images=rs.randint(0, 256, size=(B, 3072)), labels=lab, labels_random=rs.randint(10, size=B),
                     labels_biased=rs.randint(10, size=B), inv_weights=np.eye(10, dtype=np.float32)[lab],
                     labels_all=np.concatenate([lab, rs.randint(10, size=B)]))
        m.d_step(iteration=1)
        rep = m.bcr_report()
        assert np.isfinite(m.losses()[0]) and np.isfinite([rep["real"], rep["fake"]]).all() and rep["real"] > 0 and rep["fake"] > 0, rep
    finally:
        m.ctx.close()


def test_two_ranks_are_refused_before_any_gpu_work(tmp_path):
    argv = _argv(tmp_path, "b2", 1, ["--bcr_real", "10", "--bcr_fake", "10"])
    argv[argv.index("--ngpus") + 1] = "2"
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0
    assert "world_size = 2" in r.stderr.decode() and "bcr_real" in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert not os.path.exists(os.path.join(str(tmp_path), "b2"))
