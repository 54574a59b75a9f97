"""Reference learning curve of the label classifier on the class-pattern stand-in (tests/test_gpu_classifier_training.py reads
the result): the float32 PyTorch-CPU restatement of tests/classifier_ref.py, three seeds of the initialisation side by side.

Training set synthetic_cifar(12800, 1234, "templates", 20) in consecutive batches of 128, the set cycled; held out
synthetic_cifar(1000, 1235, "templates", 20) scored as ONE batch (batch-moment batch norm); lr 0.1, momentum 0.9, weight decay
1e-4, no Nesterov, no augmentation.  Writes profiles/classifier_templates_reference.json: held-out accuracy every 10 steps per seed.
CPU only, about a quarter of an hour on 16 cores.

    python scripts/classifier_reference_curve.py [--steps 250] [--seeds 0 1 2] [--out profiles/classifier_templates_reference.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_TRAIN, N_HELD, BATCH, LR, MOMENTUM, WD = 20, 12800, 1000, 128, 0.1, 0.9, 1e-4


def run_seed(args):
    seed, steps, threads = args
    import numpy as np
    import torch
    torch.set_num_threads(threads)
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from tests import classifier_ref as R
    tx, ty = D.synthetic_cifar(N_TRAIN, 1234, "templates", K)
    vx, vy = D.synthetic_cifar(N_HELD, 1235, "templates", K)
    tx, vx = R.chw_to_nhwc(tx), R.chw_to_nhwc(vx)
    P = R.init_params(seed, K, torch.float32)
    A = {k: torch.zeros_like(v) for k, v in P.items()}
    curve, losses = {}, {}
    t0 = time.time()
    for step in range(1, steps + 1):
        lo = ((step - 1) * BATCH) % N_TRAIN
        loss, _, _ = R.sgd_step(P, A, tx[lo:lo + BATCH], ty[lo:lo + BATCH], LR, MOMENTUM, WD, False)
        if step % 10 == 0:
            acc = float((np.argmax(R.softmax(P, vx), 1) == vy).mean())
            curve[str(step)], losses[str(step)] = acc, loss
            print("seed %d step %d loss %.4f held-out accuracy %.3f (%.0f s)" % (seed, step, loss, acc, time.time() - t0), flush=True)
    return seed, curve, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_templates_reference.json"))
    a = ap.parse_args()
    # a shared machine shows many more CPUs than a command may use: OMP_NUM_THREADS when set, never more than 16 in all
    cpus = min(int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1), 16)
    threads = max(1, cpus // len(a.seeds))
    with ProcessPoolExecutor(len(a.seeds)) as ex:
        res = list(ex.map(run_seed, [(s, a.steps, threads) for s in a.seeds]))
    final = [c[str(a.steps)] for _, c, _ in res]
    out = dict(what="held-out accuracy of the float32 PyTorch-CPU restatement (tests/classifier_ref.py), every 10 steps per seed",
               n_classes=K, train=[N_TRAIN, 1234, "templates"], held_out=[N_HELD, 1235, "templates"], batch=BATCH, lr=LR,
               momentum=MOMENTUM, weight_decay=WD, nesterov=False, augment=False, steps=a.steps,
               seeds={str(s): c for s, c, _ in res}, train_loss={str(s): l for s, _, l in res},
               final_min=min(final), final_max=max(final), final_spread=max(final) - min(final))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: final %s" % (a.out, final))


if __name__ == "__main__":
    main()
