"""Restatement of the label classifier and its training step for the tests: the pre-activation ResNet-32 that
``eval_cifar.LabelClassifier`` evaluates, in PyTorch on the CPU with autograd (float64 for the parity tests, float32 for the
reference learning curve), the sparse softmax cross-entropy, ``tf.train.MomentumOptimizer`` and the input augmentation in numpy.
The product never imports this module.

Variables are a dict keyed as the weight asset is (``conv2_0|conv1_in_block|conv``, ``fc|fc_weights`` ...)."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES, BLOCKS = 3, 5
BN_EPS = float(np.float32(1e-3))        # the asset's ``...|batchnorm|add|y`` scalars: float32(1e-3), not 1e-3
TRACE = None                            # a list: _bn_relu appends (name, pre-activation tensor) -- how close a batch sits to the ReLU kinks


def bn_names():
    """The 31 batch norms in execution order."""
    out = ["conv0"]
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            if not (s == 1 and b == 0):
                out.append(p + "|conv1_in_block")
            out.append(p + "|conv2_in_block")
    return out + ["fc"]


def conv_names():
    """The 31 filters in execution order."""
    out = ["conv0"]
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            out += ["conv%d_%d|conv1_in_block" % (s, b), "conv%d_%d|conv2_in_block" % (s, b)]
    return out


def decayed_names():
    return [n + "|conv" for n in conv_names()] + ["fc|fc_weights"]


def shapes(n_classes):
    """name -> shape of the 95 float arrays."""
    sh = {"conv0|conv": (3, 3, 3, 16)}
    cin = 16
    for s in range(1, STAGES + 1):
        c = 16 << (s - 1)
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            sh[p + "|conv1_in_block|conv"] = (3, 3, cin, c)
            sh[p + "|conv2_in_block|conv"] = (3, 3, c, c)
            if not (s == 1 and b == 0):
                sh[p + "|conv1_in_block|gamma"] = sh[p + "|conv1_in_block|beta"] = (cin,)
            sh[p + "|conv2_in_block|gamma"] = sh[p + "|conv2_in_block|beta"] = (c,)
            cin = c
    sh["conv0|gamma"] = sh["conv0|beta"] = (16,)
    sh["fc|gamma"] = sh["fc|beta"] = (64,)
    sh["fc|fc_weights"] = (64, n_classes)
    sh["fc|fc_bias"] = (n_classes,)
    return sh


def init_params(seed, n_classes, dtype=torch.float32):
    """He-normal filters (fan-out), gamma 1, beta 0, dense weight uniform +-1/8, bias 0 -- from torch's generator (the product draws the same
    distributions from numpy: a different stream)."""
    g = torch.Generator().manual_seed(int(seed))
    P = {}
    for name, sh in shapes(n_classes).items():
        if name.endswith("|conv"):
            P[name] = torch.randn(sh, generator=g, dtype=torch.float64) * np.sqrt(2.0 / (sh[0] * sh[1] * sh[3]))
        elif name.endswith("gamma"):
            P[name] = torch.ones(sh, dtype=torch.float64)
        elif name == "fc|fc_weights":
            P[name] = (torch.rand(sh, generator=g, dtype=torch.float64) * 2 - 1) / 8.0
        else:
            P[name] = torch.zeros(sh, dtype=torch.float64)
    return {k: v.to(dtype) for k, v in P.items()}


def _conv(x, w, stride):
    w = w.permute(3, 2, 0, 1)                      # HWIO -> OIHW
    if stride == 1:
        return F.conv2d(x, w, padding=1)
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)      # TF SAME on an even size: nothing before, one after


def _bn_relu(x, P, name, eps):
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    y = (x - mean) * torch.rsqrt(var + eps) * P[name + "|gamma"].view(1, -1, 1, 1) + P[name + "|beta"].view(1, -1, 1, 1)
    if TRACE is not None:
        TRACE.append((name, y.detach()))
    return torch.relu(y)


def shortcut_a(x):
    """Option A: 2x2 mean, then c/2 zero channels on each side (NCHW)."""
    c = x.shape[1]
    return F.pad(F.avg_pool2d(x, 2), (0, 0, 0, 0, c // 2, c // 2))


def logits(P, images_nhwc, eps=BN_EPS):
    """images [n,32,32,3] raw pixel values 0..255 -> logits [n,K]; every batch norm on the moments of this batch."""
    any_p = P["conv0|conv"]
    x = torch.as_tensor(np.asarray(images_nhwc), dtype=any_p.dtype).permute(0, 3, 1, 2)
    h = _bn_relu(_conv(x, P["conv0|conv"], 1), P, "conv0", eps)
    for s in range(1, STAGES + 1):
        for b in range(BLOCKS):
            p = "conv%d_%d" % (s, b)
            down = b == 0 and s > 1
            t = h if (s == 1 and b == 0) else _bn_relu(h, P, p + "|conv1_in_block", eps)
            c1 = _conv(t, P[p + "|conv1_in_block|conv"], 2 if down else 1)
            c2 = _conv(_bn_relu(c1, P, p + "|conv2_in_block", eps), P[p + "|conv2_in_block|conv"], 1)
            h = c2 + (shortcut_a(h) if down else h)
    feat = _bn_relu(h, P, "fc", eps).mean(dim=(2, 3))
    return feat @ P["fc|fc_weights"] + P["fc|fc_bias"]


def softmax(P, images_nhwc, eps=BN_EPS):
    with torch.no_grad():
        return torch.softmax(logits(P, images_nhwc, eps), dim=1).numpy()


def xent(lg, labels):
    """mean over rows of -log softmax(lg)[label]."""
    return F.cross_entropy(lg, torch.as_tensor(np.asarray(labels), dtype=torch.long))


def loss_and_grads(P, images_nhwc, labels, eps=BN_EPS):
    """-> (loss, accuracy of the batch, {name: gradient}) with autograd."""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    lg = logits(Q, images_nhwc, eps)
    loss = xent(lg, labels)
    loss.backward()
    acc = float((lg.detach().argmax(1).numpy() == np.asarray(labels)).mean())
    return float(loss), acc, {k: v.grad for k, v in Q.items()}


def momentum_update(w, g, accum, lr, momentum, weight_decay, nesterov, decayed, grad_scale=1.0):
    """tf.train.MomentumOptimizer on arrays / tensors, in place of nothing: returns (w, accum).  decayed: add weight_decay * w to g."""
    g = grad_scale * g + (weight_decay * w if decayed else 0.0)
    accum = momentum * accum + g
    w = w - lr * (g + momentum * accum) if nesterov else w - lr * accum
    return w, accum


def sgd_step(P, A, images_nhwc, labels, lr, momentum=0.9, weight_decay=1e-4, nesterov=False, eps=BN_EPS):
    """One training step on (P, A = momentum accumulators), both updated in place.  -> (loss, batch accuracy, gradients)."""
    loss, acc, G = loss_and_grads(P, images_nhwc, labels, eps)
    dec = set(decayed_names())
    for k in P:
        P[k], A[k] = momentum_update(P[k], G[k], A[k], lr, momentum, weight_decay, nesterov, k in dec)
    return loss, acc, G


def augment(images_chw_u8, labels_all, index, shift_flip, pad=4):
    """The input pipeline of a step in numpy.  images [N,3072] uint8 (CHW), index [n], shift_flip [n,3] = (dy, dx, flip):
    out[i, y, x] = src[y - dy, x - dx] (zeros shifted in), then mirrored left-right when flip is 1.  -> (float32 NHWC 0..255, labels)."""
    src = np.asarray(images_chw_u8).reshape(-1, 3, 32, 32)
    index, sf = np.asarray(index), np.asarray(shift_flip)
    out = np.zeros((len(index), 32, 32, 3), np.float32)
    for i, (j, (dy, dx, fl)) in enumerate(zip(index, sf)):
        assert abs(dy) <= pad and abs(dx) <= pad
        img = src[j].transpose(1, 2, 0).astype(np.float32)
        sh = np.zeros_like(img)
        ys, xs = slice(max(dy, 0), 32 + min(dy, 0)), slice(max(dx, 0), 32 + min(dx, 0))
        yo, xo = slice(max(-dy, 0), 32 + min(-dy, 0)), slice(max(-dx, 0), 32 + min(-dx, 0))
        sh[ys, xs] = img[yo, xo]
        out[i] = sh[:, ::-1] if fl else sh
    return out, np.asarray(labels_all)[index]


def chw_to_nhwc(images_chw_u8):
    return np.asarray(images_chw_u8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).astype(np.float32)
