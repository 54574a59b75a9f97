"""Reference learning curve of the MNIST label classifier on the class-pattern stand-in digits (tests/test_gpu_mnist_classifier_training.py
reads the result): a float32 PyTorch-CPU restatement of rcgan_amd/mnist_classifier.py with autograd -- relu -> max_pool2d(2) twice,
dense + relu, dropout (keep_prob 0.5, masks from torch's generator), dense, cross-entropy, TF-form Adam -- three seeds of the
initialisation (create_mnist_classifier_variables) and of the masks side by side.

Training set data_mnist.synthetic(6400, 1234, "templates") / 255 in consecutive batches of 128, the set cycled; held out
synthetic(1000, 1235, "templates") / 255 scored without dropout.  Writes profiles/mnist_classifier_templates_reference.json: held-out
accuracy every 10 steps per seed.  CPU only, under a minute on 12 cores.

    python scripts/mnist_classifier_reference_curve.py [--steps 100] [--lr 1e-3] [--seeds 0 1 2] [--out profiles/mnist_classifier_templates_reference.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TRAIN, N_HELD, BATCH, KEEP_PROB, BETA1, BETA2, EPS = 6400, 1000, 128, 0.5, 0.9, 0.999, 1e-8


def run_seed(args):
    seed, steps, lr, threads = args
    import numpy as np
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(threads)
    import rcgan_amd  # noqa: F401
    from rcgan_amd import data_mnist as DM
    from rcgan_amd.mnist_classifier import create_mnist_classifier_variables
    tx, ty = DM.synthetic(N_TRAIN, 1234, "templates")
    vx, vy = DM.synthetic(N_HELD, 1235, "templates")
    nchw = lambda a: torch.from_numpy((a / 255.).astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    tx, vx, ty = nchw(tx), nchw(vx), torch.from_numpy(ty)
    V = {n: torch.from_numpy(i.copy()).requires_grad_(True) for n, _, i in create_mnist_classifier_variables(seed)}
    M = {n: torch.zeros_like(v) for n, v in V.items()}
    S = {n: torch.zeros_like(v) for n, v in V.items()}
    gen = torch.Generator().manual_seed(1000 + seed)

    def logits(x, train):
        conv = lambda t, w, b: F.conv2d(t, w.permute(3, 2, 0, 1), b, padding=2)
        t = F.max_pool2d(torch.relu(conv(x, V["conv1|w"], V["conv1|b"])), 2)
        t = F.max_pool2d(torch.relu(conv(t, V["conv2|w"], V["conv2|b"])), 2)
        feat = torch.relu(t.permute(0, 2, 3, 1).reshape(len(x), -1) @ V["fc1|w"] + V["fc1|b"])          # NHWC order
        if train:
            feat = feat * ((torch.rand(feat.shape, generator=gen) < KEEP_PROB).float() / KEEP_PROB)
        return feat @ V["fc2|w"] + V["fc2|b"]

    curve, losses = {}, {}
    t0 = time.time()
    for step in range(1, steps + 1):
        lo = ((step - 1) * BATCH) % N_TRAIN
        loss = F.cross_entropy(logits(tx[lo:lo + BATCH], True), ty[lo:lo + BATCH])
        grads = torch.autograd.grad(loss, list(V.values()))
        with torch.no_grad():
            lr_t = lr * (1.0 - BETA2 ** step) ** 0.5 / (1.0 - BETA1 ** step)          # tf.train.AdamOptimizer
            for (n, v), g in zip(V.items(), grads):
                M[n].mul_(BETA1).add_(g, alpha=1.0 - BETA1)
                S[n].mul_(BETA2).addcmul_(g, g, value=1.0 - BETA2)
                v.sub_(lr_t * M[n] / (S[n].sqrt() + EPS))
            if step % 10 == 0:
                acc = float((logits(vx, False).argmax(1).numpy() == vy).mean())
                curve[str(step)], losses[str(step)] = acc, float(loss)
                print("seed %d step %d loss %.4f held-out accuracy %.3f (%.0f s)" % (seed, step, float(loss), acc, time.time() - t0), flush=True)
    return seed, curve, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnist_classifier_templates_reference.json"))
    a = ap.parse_args()
    # a shared machine shows many more CPUs than a command may use: OMP_NUM_THREADS when set, never more than 16 in all
    cpus = min(int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1), 16)
    threads = max(1, cpus // len(a.seeds))
    with ProcessPoolExecutor(len(a.seeds)) as ex:
        res = list(ex.map(run_seed, [(s, a.steps, a.lr, threads) for s in a.seeds]))
    final = [c[str(a.steps)] for _, c, _ in res]
    out = dict(what="held-out accuracy of the float32 PyTorch-CPU restatement of the MNIST label classifier, every 10 steps per seed",
               n_classes=10, train=[N_TRAIN, 1234, "templates"], held_out=[N_HELD, 1235, "templates"], batch=BATCH, lr=a.lr,
               keep_prob=KEEP_PROB, beta1=BETA1, beta2=BETA2, eps=EPS, steps=a.steps,
               seeds={str(s): c for s, c, _ in res}, train_loss={str(s): l for s, _, l in res},
               final_min=min(final), final_max=max(final), final_spread=max(final) - min(final))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: final %s" % (a.out, final))


if __name__ == "__main__":
    main()
