"""The short synthetic training run the metric tests start as a process of its own: ``train_cifar.main`` on class-pattern images, 8
images per batch, none of the reference's own evaluations, with every construction of a LabelClassifier counted."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the training entry with every construction of a LabelClassifier counted
COUNTING = ("import sys; sys.path.insert(0, %r); import rcgan_amd; from rcgan_amd import eval_cifar, train_cifar; built = []; "
            "init = eval_cifar.LabelClassifier.__init__; "
            "eval_cifar.LabelClassifier.__init__ = lambda self, *a, **k: (built.append(1), init(self, *a, **k))[1]; "
            "train_cifar.main(sys.argv[1:]); print('label classifiers built: %%d' %% len(built))" % ROOT)


def launch(tmp_path, extra, expt, niters=4, script=None):
    """Runs ``niters`` iterations with the flags ``extra`` in <tmp_path>/<expt>, through COUNTING or (script: a path) through that
    launcher.  -> (the log's text, LabelClassifiers built -- None under a script, which does not count).  The log is removed: a
    second run under the same name starts a fresh one."""
    log = os.path.join(str(tmp_path), "log_%s.txt" % expt)
    argv = [sys.executable] + (["-c", COUNTING] if script is None else [script]) + [
        "--algorithm", "rcgan", "--alpha", "0.6", "--log_file", log,
        "--parent_dir", str(tmp_path), "--expt_dir", expt, "--ngpus", "1", "--multi_gpu_multi_batch", "--niters", str(niters), "--batch_size", "8",
        "--synthetic", "--synthetic_kind", "templates", "--sample_freq", "0", "--inception_freq", "0",
        "--generated_label_accuracy_freq", "0", "--early_checkpoint_every", "4"] + extra
    r = subprocess.run(argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    built = re.search(r"label classifiers built: (\d+)", r.stdout.decode())
    text = open(log).read()
    os.remove(log)
    return text, int(built.group(1)) if built else None
