"""The sliced Wasserstein distance on Laplacian-pyramid patch descriptors (Karras et al. 2018, section 5) restated in float64 numpy:
the yardstick of csrc/swd.hip and rcgan_amd/swd.py.  Images: uint8 NHWC, c 1 or 3, h and w each 28 or 32.

  G0 = x, G1 = down(G0), G2 = down(G1);    L0 = G0 - up(G1), L1 = G1 - up(G2), L2 = G2
  down: [1,4,6,4,1]/16 along each axis, mirror boundary without repeating the edge, even indices kept
  up:   zero-insert to twice the size, then [1,4,6,4,1]/8 along each axis, the same boundary
  descriptors of level l: the 7 x 7 x c neighbourhoods centred on y = 3, 3 + stride_l, ... <= s_h - 4 (likewise x), strides 4, 2, 1,
  elements in the order (dy, dx, channel); normalised per set and channel over all descriptor entries (ddof 0; 1 / 0 := 0)
  SWD_l = 1e3 * mean over directions of mean_i |sort(A w)_i - sort(B w)_i|

The directions are handed in as fp32 (the fp32 values are the definition) and widened here."""
import numpy as np

TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
STRIDES = (4, 2, 1)
PATCH = 7
U = 2.0 ** -24
DELTA = (0.0, 7 * U * 255, 0.0)          # |level value of csrc/swd.hip - exact| (its header)


def _mirror(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _filter(x, axis, scale):
    """The five taps / scale along ``axis`` at every index, mirror boundary."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
    n = x.shape[0]
    out = sum(TAPS[t] * x[_mirror(np.arange(n) + t - 2, n)] for t in range(5)) / scale
    return np.moveaxis(out, 0, axis)


def down(x):
    """[n,h,w,c] -> [n,h/2,w/2,c]."""
    return _filter(_filter(x, 1, 16.0), 2, 16.0)[:, ::2, ::2]


def up(g):
    """[n,h,w,c] -> [n,2h,2w,c]."""
    g = np.asarray(g, np.float64)
    u = np.zeros((g.shape[0], 2 * g.shape[1], 2 * g.shape[2], g.shape[3]))
    u[:, ::2, ::2] = g
    return _filter(_filter(u, 1, 8.0), 2, 8.0)


def pyramid(x):
    """uint8 [n,h,w,c] -> [L0, L1, L2], float64."""
    g0 = np.asarray(x, np.float64)
    g1 = down(g0)
    g2 = down(g1)
    return [g0 - up(g1), g1 - up(g2), g2]


def lattice(size, stride):
    return np.arange(3, size - 3, stride)


def descriptors(level, stride):
    """[n,s_h,s_w,c] -> [n, n_pos, 49 c]: raw neighbourhoods in the order (dy, dx, channel), positions row-major."""
    n, sh, sw, c = level.shape
    out = [level[:, y - 3:y + 4, x - 3:x + 4, :].reshape(n, -1) for y in lattice(sh, stride) for x in lattice(sw, stride)]
    return np.stack(out, axis=1)


def moments(desc, c):
    """[m, 49 c] descriptor rows of one segment -> (mean [c], deviation [c]) over all entries of a channel, two-pass."""
    d = desc.reshape(-1, c)
    if len(d) == 0:
        return np.zeros(c), np.zeros(c)
    mean = d.mean(axis=0)
    return mean, np.sqrt(((d - mean) ** 2).mean(axis=0))


def normalise(desc, c):
    mean, dev = moments(desc, c)
    rstd = np.where(dev > 0, 1.0 / np.where(dev > 0, dev, 1.0), 0.0)
    return ((desc.reshape(-1, c) - mean) * rstd).reshape(desc.shape)


def level_descriptors(x, level):
    """uint8 [n,h,w,c] -> the RAW descriptors of pyramid level ``level`` as rows [n * n_pos, 49 c], image-major."""
    d = descriptors(pyramid(x)[level], STRIDES[level])
    return d.reshape(-1, d.shape[2])


def projections(x, level, dirs):
    """-> float64 [n_dir, n * n_pos]: the normalised descriptors of the set x on the directions (what rcgan_swd_project computes
    for one segment)."""
    c = np.shape(x)[3]
    return np.asarray(dirs, np.float64) @ normalise(level_descriptors(x, level), c).T


def projection_bound(x, level, dirs):
    """The derived bound of csrc/swd.hip on |proj_gpu - projections(x, level, dirs)|, per entry [n_dir, n * n_pos]."""
    c = np.shape(x)[3]
    raw = level_descriptors(x, level)
    mean, dev = moments(raw, c)
    live = dev > 0
    if not live.any():
        return np.zeros((len(dirs), len(raw)))
    r_max = float((1.0 / dev[live]).max())
    delta = DELTA[level]
    assert delta * r_max <= 1e-3
    a = 2 * delta + 765 * U + 2.0 ** -40
    q = (raw.reshape(-1, c) ** 2).mean(axis=0)
    eps64 = 2.0 ** -45 * float((q[live] / dev[live] ** 2).max())
    d = 49 * c
    s_abs = np.abs(np.asarray(dirs, np.float64)) @ np.abs(normalise(raw, c)).T
    return (1 + 1e-5) * (r_max * a * np.sqrt(d) + (delta * r_max + (d + 2) * U / (1 - d * U) + eps64) * s_abs)


def sliced(pa, pb):
    """Projections [n_dir, m] of two sets of equally many descriptors -> 1e3 * mean_d mean_i |sort(pa)_i - sort(pb)_i|."""
    if pa.shape != pb.shape:
        raise ValueError("sliced: %s against %s" % (pa.shape, pb.shape))
    return 1e3 * float(np.abs(np.sort(pa, axis=1) - np.sort(pb, axis=1)).mean())


def swd(xa, xb, dirs):
    """uint8 [m,h,w,c] twice, dirs: fp32 [3, n_dir, 49 c] -> float64 [3], the distance per level."""
    if len(xa) != len(xb):
        raise ValueError("swd: %d against %d images" % (len(xa), len(xb)))
    return np.array([sliced(projections(xa, l, dirs[l]), projections(xb, l, dirs[l])) for l in range(3)])


def first_rows(labels, n_classes, take):
    """Row indices: class by class the first take[c] rows with label c."""
    lab = np.asarray(labels).reshape(-1)
    return [np.flatnonzero(lab == c)[:take[c]] for c in range(n_classes)]


def evaluate(real, real_labels, gen, gen_labels, n_classes, dirs):
    """The evaluator restated: -> dict(pooled [3], per_class [K,3] (nan where a side has fewer than 2 images), floor_pooled [3],
    floor_per_class [K,3], counts [K])."""
    K = int(n_classes)
    rl, gl = np.asarray(real_labels).reshape(-1), np.asarray(gen_labels).reshape(-1)
    rk, gk = np.flatnonzero((rl >= 0) & (rl < K)), np.flatnonzero((gl >= 0) & (gl < K))
    real, rl, gen, gl = np.asarray(real)[rk], rl[rk], np.asarray(gen)[gk], gl[gk]
    r_c, g_c = np.bincount(rl, minlength=K), np.bincount(gl, minlength=K)
    m = min(len(gen), len(real))
    out = dict(pooled=swd(gen[:m], real[:m], dirs), per_class=np.full((K, 3), np.nan), floor_per_class=np.full((K, 3), np.nan))
    mf = min(len(gen), len(real) // 2)
    out["floor_pooled"] = swd(real[:mf], real[mf:2 * mf], dirs)
    take, half = np.minimum(g_c, r_c), np.minimum(g_c, r_c // 2)
    g_rows, r_rows, f_rows = first_rows(gl, K, take), first_rows(rl, K, take), first_rows(rl, K, 2 * half)
    for c in range(K):
        if min(g_c[c], r_c[c]) >= 2:
            out["per_class"][c] = swd(gen[g_rows[c]], real[r_rows[c]], dirs)
        if half[c] >= 2:
            out["floor_per_class"][c] = swd(real[f_rows[c][:half[c]]], real[f_rows[c][half[c]:]], dirs)
    out["counts"] = take
    return out
