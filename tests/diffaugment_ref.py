"""DiffAugment as include/rcgan_hip.h defines it (rcgan_diffaugment_fwd), restated with torch: the reference of the CPU property tests
and of the GPU tests (float64, the adjoint by autograd).

The discrete choices -- translation, cutout window -- and b, s, k are formed from u in float32, as the definition says ("the product
in fp32"): a float64 product could land on the other side of a floor() at u = 0.99999994.  Everything after that runs in x's dtype.
"""
import numpy as np
import torch
import torch.nn.functional as F

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
POLICIES = (1, 2, 3, 4, 5, 6, 7)
U_MAX = float(np.float32(1.0) - np.float32(2.0 ** -24))      # 0.99999994, the largest float32 below 1


def _index(u, count):
    """min(floor(u * count), count - 1), the product in float32."""
    return min(int(np.floor(np.float32(u) * np.float32(count))), count - 1)


def params(u_row, h, w, policy):
    """-> dict(b, s, k, ty, tx, rows=(r0, r1), cols=(c0, c1)); rows / cols inclusive, None without CUTOUT."""
    u = np.asarray(u_row, np.float32)
    p = dict(b=float(u[0] - np.float32(0.5)), s=float(np.float32(2.0) * u[1]), k=float(u[2] + np.float32(0.5)),
             ty=0, tx=0, rows=None, cols=None)
    if policy & TRANSLATION:
        sh, sw = (h + 4) // 8, (w + 4) // 8
        p["ty"] = _index(u[3], 2 * sh + 1) - sh
        p["tx"] = _index(u[4], 2 * sw + 1) - sw
    if policy & CUTOUT:
        oy, ox = _index(u[5], h + 1), _index(u[6], w + 1)
        p["oy"], p["ox"] = oy, ox
        p["rows"] = (max(oy - h // 4, 0), min(oy + h // 4 - 1, h - 1))
        p["cols"] = (max(ox - w // 4, 0), min(ox + w // 4 - 1, w - 1))
    return p


def augment_one(x, u_row, policy):
    """x [h, w, 3] torch (any float dtype, may require grad) -> A_u(x)."""
    h, w, c = x.shape
    assert c == 3
    p = params(u_row, h, w, policy)
    if policy & COLOR:
        x = x + p["b"]
        m = x.mean(dim=-1, keepdim=True)
        x = (x - m) * p["s"] + m
        M = x.mean()
        x = (x - M) * p["k"] + M
    if policy & TRANSLATION:
        sh, sw = (h + 4) // 8, (w + 4) // 8
        xp = F.pad(x, (0, 0, sw, sw, sh, sh))
        x = xp[sh + p["ty"]:sh + p["ty"] + h, sw + p["tx"]:sw + p["tx"] + w]
    if policy & CUTOUT:
        mask = torch.ones(h, w, 1, dtype=x.dtype)
        mask[p["rows"][0]:p["rows"][1] + 1, p["cols"][0]:p["cols"][1] + 1] = 0
        x = x * mask
    return x


def diffaugment(x, u, policy):
    """x [n, h, w, 3] torch, u [n, 8] -> [n, h, w, 3]."""
    u = np.asarray(u, np.float32)
    assert u.shape == (x.shape[0], 8), u.shape
    return torch.stack([augment_one(x[i], u[i], policy) for i in range(x.shape[0])])


def support(u, h, w, policy):
    """bool [n, h, w]: the INPUT pixels some output pixel reads (not shifted out of the frame, their reader not cut out).  Without
    COLOR the gradient is exactly zero outside it."""
    u = np.asarray(u, np.float32)
    out = np.zeros((len(u), h, w), bool)
    for i in range(len(u)):
        p = params(u[i], h, w, policy)
        for r in range(h):
            for c in range(w):
                orow, ocol = r - p["ty"], c - p["tx"]
                if not (0 <= orow < h and 0 <= ocol < w):
                    continue
                if p["rows"] is not None and p["rows"][0] <= orow <= p["rows"][1] and p["cols"][0] <= ocol <= p["cols"][1]:
                    continue
                out[i, r, c] = True
    return out


def extreme_rows():
    """The hand-built draws: every slot at 0 and at U_MAX around a mid-range row (u1 = 0 is s = 0, u2 = 0 is k = 0.5), and every
    combination of the translation extremes with the cutout extremes (the shifted-in zeros and the window then overlap)."""
    rows = []
    for j in range(7):
        for v in (0.0, U_MAX):
            r = np.full(8, 0.5, np.float32)
            r[j] = v
            rows.append(r)
    for a in (0.0, U_MAX):
        for b in (0.0, U_MAX):
            for c in (0.0, U_MAX):
                for d in (0.0, U_MAX):
                    r = np.full(8, 0.5, np.float32)
                    r[3], r[4], r[5], r[6] = a, b, c, d
                    rows.append(r)
    return np.stack(rows)


def draws(n, seed):
    """u [m, 8] for launches of n rows: the extreme rows, then random ones (at least six) up to a multiple of n."""
    ext = extreme_rows()
    m = -(-(len(ext) + 6) // n) * n
    rs = np.random.RandomState(seed)
    rnd = rs.uniform(0.0, 1.0, size=(m - len(ext), 8)).astype(np.float32)
    rnd = np.minimum(rnd, np.float32(U_MAX))
    return np.concatenate([ext, rnd]).astype(np.float32)
