"""Reference numbers for the forward-corrected label classifier under label noise (tests/test_gpu_forward_training.py reads the
result): the float32 PyTorch-CPU restatement of tests/classifier_ref.py with the loss of tests/forward_xent_ref.py, three seeds of the
initialisation side by side.

Training set synthetic_cifar(12800, 1234, "templates", 20), its labels corrupted ONCE through the one-coin matrix C_ALPHA(0.6, 20)
(data.noisy_labels, RandomState(label_seed)), in consecutive batches of 128, the set cycled; forward loss with that known matrix; lr 0.1,
momentum 0.9, weight decay 1e-4, no Nesterov, no augmentation.  Two numbers per seed: accuracy against the CLEAN labels of held-out
synthetic_cifar(1000, 1235, "templates", 20) scored as ONE batch, and label-recovery accuracy on the first 2000 training images (the
arg-max of softmax(z)[y] C[y, noisy] against their clean labels, two batches of 1000, every batch norm on the moments of its batch).
Writes profiles/classifier_forward_reference.json.  CPU only, at most 16 threads; about six minutes on 8 cores.

    python scripts/classifier_forward_reference_curve.py [--steps 250] [--seeds 0 1 2] [--out profiles/classifier_forward_reference.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_TRAIN, N_HELD, N_RECOVER, BATCH, LR, MOMENTUM, WD = 20, 12800, 1000, 2000, 128, 0.1, 0.9, 1e-4
ALPHA, LABEL_SEED = 0.6, 7


def run_seed(args):
    seed, steps, threads = args
    import numpy as np
    import torch
    torch.set_num_threads(threads)
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data as D
    from tests import classifier_ref as R
    from tests import forward_xent_ref as FR
    tx, ty = D.synthetic_cifar(N_TRAIN, 1234, "templates", K)
    vx, vy = D.synthetic_cifar(N_HELD, 1235, "templates", K)
    tx, vx = R.chw_to_nhwc(tx), R.chw_to_nhwc(vx)
    Cm = D.C_ALPHA(ALPHA, K)
    noisy = D.noisy_labels(ty, Cm, np.random.RandomState(LABEL_SEED))
    P = R.init_params(seed, K, torch.float32)
    A = {k: torch.zeros_like(v) for k, v in P.items()}
    held, recovery, losses = {}, {}, {}
    t0 = time.time()
    for step in range(1, steps + 1):
        lo = ((step - 1) * BATCH) % N_TRAIN
        loss, _, _ = FR.sgd_step(P, A, tx[lo:lo + BATCH], noisy[lo:lo + BATCH], Cm, LR, MOMENTUM, WD, False)
        if step % 10 == 0:
            held[str(step)], losses[str(step)] = float((np.argmax(R.softmax(P, vx), 1) == vy).mean()), loss
        if step % 50 == 0:
            rec, _ = FR.recover(P, tx[:N_RECOVER], noisy[:N_RECOVER], Cm)
            recovery[str(step)] = float((rec == ty[:N_RECOVER]).mean())
            print("seed %d step %d loss %.4f held-out accuracy %.3f recovery accuracy %.3f (%.0f s)"
                  % (seed, step, loss, held[str(step)], recovery[str(step)], time.time() - t0), flush=True)
    return seed, held, recovery, losses, float((noisy == ty).mean()), float((noisy[:N_RECOVER] == ty[:N_RECOVER]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_forward_reference.json"))
    a = ap.parse_args()
    # a shared machine shows many more CPUs than a command may use: OMP_NUM_THREADS when set, never more than 16 in all
    cpus = min(int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1), 16)
    threads = max(1, cpus // len(a.seeds))
    with ProcessPoolExecutor(len(a.seeds)) as ex:
        res = list(ex.map(run_seed, [(s, a.steps, threads) for s in a.seeds]))
    held = [r[1][str(a.steps)] for r in res]
    rec = [r[2][str(a.steps)] for r in res]
    out = dict(what="float32 PyTorch-CPU restatement (tests/classifier_ref.py + tests/forward_xent_ref.py) trained on noisy labels with the "
                    "forward-corrected loss and the known matrix: held-out accuracy against clean labels every 10 steps, label-recovery "
                    "accuracy on the first n_recover training images every 50, per seed",
               n_classes=K, train=[N_TRAIN, 1234, "templates"], held_out=[N_HELD, 1235, "templates"], n_recover=N_RECOVER, batch=BATCH, lr=LR,
               momentum=MOMENTUM, weight_decay=WD, nesterov=False, augment=False, steps=a.steps, alpha=ALPHA, label_seed=LABEL_SEED,
               noisy_agreement=res[0][4], noisy_agreement_recover=res[0][5],
               held_out_accuracy={str(r[0]): r[1] for r in res}, recovery_accuracy={str(r[0]): r[2] for r in res},
               train_loss={str(r[0]): r[3] for r in res},
               held_out_final_min=min(held), held_out_final_max=max(held), held_out_final_spread=max(held) - min(held),
               recovery_final_min=min(rec), recovery_final_max=max(rec), recovery_final_spread=max(rec) - min(rec))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: held-out %s, recovery %s" % (a.out, held, rec))


if __name__ == "__main__":
    main()
