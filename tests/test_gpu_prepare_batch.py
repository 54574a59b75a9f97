"""Batched filter preparation (rcgan_conv_prepare_batch / _riders / _frags: conv_prepare_batch_kernel) against a numpy encoder of
the documented layouts, at the limits of the ABI: 1 to 97 items (one to three launches), the three item kinds in one launch, 8 and
9 summed phase filters, and 48 items + 8 phase filters + 12 fragment copies + both riders in ONE launch (70 rows).

Encoded in numpy (no other device route is called): the 16-bit rows wt[co][t*Cin+ci] / wd[ci][(T-1-t)*Cout+co], the summed
phase / gather filters of both families, the fragment-major copies (frag_index), the fp32 copies, the image-end layouts
(wK / wS, the comment above img_prepare_elem) and the label embeddings.

Every destination is filled with a sentinel (0xFF bytes: a NaN in fp32, bf16 and fp16) and framed by guard bytes -- the padding
rcgan_conv_prepared_bytes reserves plus GUARD_BYTES allocated on each side -- before the launch.  Afterwards no sentinel may be
left inside an output and no byte outside the outputs may have changed.

Tolerances (none is loosened per case):
  single-weight 16-bit elements (wt, wd, image-end layouts, fragment copies): bit-equal to round16(fp32(w) * fp32(1 / fp32(sigma)))
      emulated in numpy, and within 1 ulp16 of round16(w / sigma) in float64.  round16 = round to nearest even to bf16
      (f32_to_bf16) in the default build, to fp16 in the RCGAN_HALF_FP16 build.  In the fp16 build the compiler contracts
      f32_to_bf16(w * inv) into v_fma_mixlo_f16, which rounds the exact product once: an element there may instead equal
      fp16(fp32(w) * fp32(1 / fp32(sigma)) in exact arithmetic), the other deterministic result (they differ only where
      rounding to fp32 first moves the value across an fp16 rounding boundary)
  fp32 copies: bit-equal to the fp32 emulation, and within 1 ulp32 of float64
  summed phase / gather filters: |got - S| <= 0.5 ulp16(S) + 4 * 2^-24 * sum|terms|, S = the float64 sum of the taps (x 1/4 in
      the mean-pool family)
  label embeddings: 2e-5 of max|ref| (float64 reference), as test_label_embeddings_ride_in_filter_preparation
  step inputs: bit-equal to the same rider in a 1-item launch; the pool bit-equal to numpy's fp32 sum of the stored pixels; each
      stored pixel within half a storage ulp of 2 (img / 256 - .5) + U[lo, hi); the fill all zeros; the random stream moved
      on by exactly n * 3072 / 4 quads"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import make_ctx

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xFF, 0x5A
GUARD_BYTES = 1024         # allocated on each side of every destination (a multiple of 256: the destinations stay aligned)
SIGMA = 1.37               # not a power of two: 1 / sigma is rounded
SINGLE_ULP16 = 1.0         # single-weight 16-bit elements against float64, in ulp16
SUM_HALF_ULP16, SUM_REL32 = 0.5, 4 * 2.0 ** -24     # summed filters: 0.5 ulp16(S) + 4 * 2^-24 * sum|terms|
EMBED_TOL = 2e-5
MAX_ITEMS, MAX_PHASE_RIDE, MAX_FRAGS = 48, 8, 12    # per launch (conv_prepare_batch_launch, rcgan_conv_prepare_batch_frags)


@pytest.fixture(scope="module", params=["f32", "bf16", "f16"])
def dev(request):
    ctx = make_ctx(request.param, arena=1 << 26)
    yield ctx, request.param
    ctx.close()


# ---------------------------------------------------------------------------------------------------------- number formats
def round16_bits(mode, a):
    """fp32 values -> raw bits of the build's 16-bit format, round to nearest even."""
    a = np.ascontiguousarray(a, np.float32)
    if mode == "f16":
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def decode16(mode, bits):
    if mode == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ulp16(mode, x):
    """Spacing of the 16-bit format at |x| (bf16: 8 significand bits; fp16: 11, subnormal spacing 2^-24)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    u = np.ldexp(1.0, e - (11 if mode == "f16" else 8))
    tiny = 2.0 ** -24 if mode == "f16" else 2.0 ** -133
    return np.where(x == 0, tiny, np.maximum(u, tiny))


def round16_64(mode, x):
    u = ulp16(mode, x)
    return np.round(x / u) * u          # half to even


def bits_of(body, off, count, size):
    return body[off:off + count * size].view(np.uint16 if size == 2 else np.uint32)


# ---------------------------------------------------------------------------------------------------------- layouts
def mfma_rows(W):
    """W [T][Cin][Cout] -> wt [Cout][T*Cin] (wt[co][t*Cin+ci]) and the rotated wd [Cin][T*Cout] (wd[ci][(T-1-t)*Cout+co])."""
    T, cin, cout = W.shape
    return W.transpose(2, 0, 1).reshape(cout, T * cin), W[::-1].transpose(1, 0, 2).reshape(cin, T * cout)


def tap_classes(kind):
    """Tap sets of the summed filters (comment above phase_taps2): two[(ph, a)] = kernel rows of row class a of phase ph,
    four[u] = kernel rows of tap u of the 4x4 stride-2 (gather) form."""
    if kind == 0:                                    # upsample -> conv
        return {(0, 0): [0], (0, 1): [1, 2], (1, 0): [0, 1], (1, 1): [2]}, [[2], [1, 2], [0, 1], [0]]
    P = [[0], [0, 1], [1, 2], [2]]                   # conv -> mean pool
    return {(0, 0): P[3], (0, 1): P[1], (1, 0): P[2], (1, 1): P[0]}, P


def phase_layouts(W3, kind):
    """W3 [3][3][Cin][Cout] float64 (already / sigma) -> the two summed layouts in memory order, each as (S, sum|terms|):
    phase [ph*2+pw][O][(a*2+b)*R + r] and gather [O][(u*4+v)*R + r]; kind 0: the phase layout first (O = Cout, R = Cin) and the
    gather layout behind it (O = Cin, R = Cout); kind 1: gather (O = Cout, R = Cin) first, phase (O = Cin, R = Cout) behind, x 1/4."""
    two, four = tap_classes(kind)
    scale = 0.25 if kind == 1 else 1.0

    def tsum(khs, kws):
        s = sum(W3[kh, kw] for kh in khs for kw in kws)
        a = sum(np.abs(W3[kh, kw]) for kh in khs for kw in kws)
        return s * scale, a * scale

    out = []
    for part in (0, 1):          # S, then sum|terms|
        ph = np.stack([np.stack([tsum(two[(p >> 1, ab >> 1)], two[(p & 1, ab & 1)])[part] for ab in range(4)]) for p in range(4)])
        g = np.stack([tsum(four[uv >> 2], four[uv & 3])[part] for uv in range(16)])       # [uv][Cin][Cout]
        if kind == 0:
            out.append((ph.transpose(0, 3, 1, 2).ravel(), g.transpose(1, 0, 2).ravel()))   # [phase][co][ab][ci], [ci][uv][co]
        else:
            out.append((g.transpose(2, 0, 1).ravel(), ph.transpose(0, 2, 1, 3).ravel()))   # [co][uv][ci], [phase][ci][ab][co]
    (s0, s1), (a0, a1) = out
    return (s0, a0), (s1, a1)


def image_end_layout(W, side):
    """The extra region of an image-end item (comment above img_prepare_elem): wK [Cb][32] then wS [T][16][Cb], zero-padded.
    side 1 (cin small): wK[n][t*Cs+c] = W[t][c][n], wS[t][j][co] = W[T-1-t][j][co];
    side 2 (cout small): wK[ci][t*Cs+co] = W[T-1-t][ci][co], wS[t][j][ci] = W[t][ci][j]."""
    T, cin, cout = W.shape
    cs, cb = (cin, cout) if side == 1 else (cout, cin)
    wk = np.zeros((cb, 32), W.dtype)
    ws = np.zeros((T, 16, cb), W.dtype)
    for t in range(T):
        for c in range(cs):
            wk[:, t * cs + c] = W[t, c, :] if side == 1 else W[T - 1 - t, :, c]
            ws[t, c, :] = W[T - 1 - t, c, :] if side == 1 else W[t, :, c]
    return np.concatenate([wk.ravel(), ws.ravel()])


def frag_encode(M, ctn, ss):
    """Rows [R][K] -> the fragment-major copy [block of 16*ctn rows][slice][step ss][tile ctn][lane 64][8] (frag_index)."""
    R, K = M.shape
    nsl = K // 32 // ss
    row, k = np.arange(R)[:, None], np.arange(K)[None, :]
    blk, ct, r = row // (16 * ctn), (row % (16 * ctn)) >> 4, row & 15
    ks = k >> 5
    sl, s, kc, e = ks // ss, ks % ss, (k >> 3) & 3, k & 7
    idx = (((((blk * nsl + sl) * ss + s) * ctn + ct) * 64 + kc * 16 + r) * 8 + e).ravel()
    assert np.array_equal(np.bincount(idx, minlength=R * K), np.ones(R * K)), "frag_index is not a permutation"
    out = np.empty(R * K, M.dtype)
    out[idx] = M.ravel()
    return out


# ---------------------------------------------------------------------------------------------------------- destinations
class Dest:
    """nbytes on the device framed by GUARD_BYTES on each side.  outs: [(byte offset, byte count)] the launch must write; they hold
    the sentinel, every other byte GUARD (or init: [(byte offset, array)]) and must come back unchanged."""

    def __init__(self, nbytes, outs, init=()):
        host = np.full(2 * GUARD_BYTES + nbytes, GUARD, np.uint8)
        for off, n in outs:
            host[GUARD_BYTES + off:GUARD_BYTES + off + n] = SENTINEL
        for off, arr in init:
            b = np.ascontiguousarray(arr).view(np.uint8).ravel()
            host[GUARD_BYTES + off:GUARD_BYTES + off + b.size] = b
        self.host, self.nbytes, self.outs = host, nbytes, outs
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + GUARD_BYTES

    def fetch(self):
        """(the nbytes between the guards, indices into the frame of bytes outside the outputs that changed)"""
        got = self.t.cpu().numpy()
        keep = np.ones(got.size, bool)
        for off, n in self.outs:
            keep[GUARD_BYTES + off:GUARD_BYTES + off + n] = False
        return got[GUARD_BYTES:GUARD_BYTES + self.nbytes].copy(), np.flatnonzero((got != self.host) & keep)


class Report:
    """Collects every failure of one case, so that a failing case lists all outputs that are wrong."""

    def __init__(self, mode):
        self.mode, self.errs = mode, []

    def fetch(self, what, dest):
        body, changed = dest.fetch()
        if changed.size:
            self.errs.append("%s: %d bytes outside the outputs changed (first at frame byte %d)" % (what, changed.size, changed[0]))
        return body

    def sentinels(self, what, got):
        left = int((got == (0xFFFF if got.dtype == np.uint16 else 0xFFFFFFFF)).sum())
        if left:
            self.errs.append("%s: %d of %d elements still hold the sentinel" % (what, left, got.size))
        return left == 0

    def single16(self, what, got, src, inv32, sig64):
        """16-bit elements each of one weight: src = the fp32 weights in layout order (zeros where the layout pads)."""
        if not self.sentinels(what, got):
            return
        want = round16_bits(self.mode, src * inv32)
        bad = got != want
        if self.mode == "f16":
            # the fp16 build contracts the product and the conversion into v_fma_mixlo_f16: the exact product rounded once to
            # fp16 (a product of two fp32 values is exact in float64, and numpy rounds float64 -> fp16 directly)
            once = (src.astype(np.float64) * np.float64(inv32)).astype(np.float16).view(np.uint16)
            bad &= got != once
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            self.errs.append("%s: %d elements differ from round16(fp32(w) * fp32(1/sigma)); first [%d] got %#06x want %#06x"
                             % (what, int(bad.sum()), i, got[i], want[i]))
        r = round16_64(self.mode, src.astype(np.float64) / sig64)
        err = np.abs(decode16(self.mode, got) - r) / ulp16(self.mode, r)
        if err.max() > SINGLE_ULP16:
            self.errs.append("%s: %.2f ulp16 from round16(w / sigma) in float64 (> %g)" % (what, err.max(), SINGLE_ULP16))

    def single32(self, what, got, src, inv32, sig64):
        if not self.sentinels(what, got):
            return
        want = (src * inv32).astype(np.float32).view(np.uint32)
        if not np.array_equal(got, want):
            self.errs.append("%s: %d fp32 elements differ from fp32(w) * fp32(1/sigma)" % (what, int((got != want).sum())))
        g = got.view(np.float32)
        err = np.abs(g.astype(np.float64) - src.astype(np.float64) / sig64) / np.spacing(np.abs(g))
        if err.max() > 1.0:
            self.errs.append("%s: %.2f ulp32 from w / sigma in float64" % (what, err.max()))

    def summed16(self, what, got, S, A):
        if not self.sentinels(what, got):
            return
        err = np.abs(decode16(self.mode, got) - S) - (SUM_HALF_ULP16 * ulp16(self.mode, S) + SUM_REL32 * A)
        if err.max() > 0:
            i = int(np.argmax(err))
            self.errs.append("%s: %d elements outside 0.5 ulp16(S) + 4*2^-24*sum|terms|; worst [%d] got %r, S %r"
                             % (what, int((err > 0).sum()), i, decode16(self.mode, got[i:i + 1])[0], S[i]))

    def done(self):
        assert not self.errs, "\n".join(self.errs)


# ---------------------------------------------------------------------------------------------------------- items
CIN_SMALL_SIDE, COUT_SMALL_SIDE = 1, 2


class Item:
    """One filter: spec = (cin, cout, k, hw, flags, kind on the 16-bit path: "mfma" / "img1" / "img2" / "plain")."""

    def __init__(self, L, ctx, mode, rs, spec, with_sigma):
        cin, cout, k, hw, flags, kind16 = spec
        self.cin, self.cout, self.T, self.flags = cin, cout, k * k, flags
        self.kind = "plain" if mode == "f32" else kind16
        self.phase = self.kind == "mfma" and k == 3 and bool(flags & (L.CONV_IN_UPSAMPLE2X | L.CONV_OUT_MEANPOOL2))
        self.pool = bool(flags & L.CONV_OUT_MEANPOOL2)
        self.desc = L.ConvDesc(1, hw, hw, cin, cout, k, k, 1, ctx.act_dtype, flags)
        self.w = (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32)
        self.w_dev = torch.from_numpy(self.w).cuda()
        self.sig32 = np.float32(SIGMA) if with_sigma else None
        self.sig_dev = torch.tensor([SIGMA], dtype=torch.float32).cuda() if with_sigma else None
        self.inv32 = np.float32(1) / self.sig32 if with_sigma else np.float32(1)
        self.sig64 = float(self.sig32) if with_sigma else 1.0
        E = self.T * cin * cout
        self.img_off = (E * 4 + 255) // 256 * 256
        cb = cout if self.kind == "img1" else cin
        self.img_elems = cb * 32 + self.T * 16 * cb
        # the item's kind, confirmed through the buffer size the ABI asks for (mfma_eligible / img_side decide it)
        want = {"mfma": 4 * E + (64 * cin * cout if self.phase else 0) + 256, "img1": self.img_off + 2 * self.img_elems + 256,
                "img2": self.img_off + 2 * self.img_elems + 256, "plain": 4 * E + 256}[self.kind]
        self.nbytes = ctx.lib.rcgan_conv_prepared_bytes(C.byref(self.desc))
        assert self.nbytes == want, ("item kind", spec, self.kind, self.nbytes, want)
        if self.kind == "mfma":
            outs = [(0, 4 * E)] + ([(4 * E, 64 * cin * cout)] if self.phase else [])
        else:
            outs = [(0, 4 * E)] + ([(self.img_off, 2 * self.img_elems)] if self.kind != "plain" else [])
        self.dest = Dest(self.nbytes, outs)
        self.frags = []

    def prepare_item(self, L):
        return L.PrepareItem(self.desc, self.w_dev.data_ptr(), self.sig_dev.data_ptr() if self.sig_dev is not None else None,
                             self.dest.ptr)

    def add_frag(self, L, ctn, ss):
        n = self.T * self.cin * self.cout * 2
        f = (ctn, ss, Dest(n, [(0, n)]), Dest(n, [(0, n)]))
        self.frags.append(f)
        return f

    def check(self, rep, name):
        W = self.w.reshape(self.T, self.cin, self.cout)
        E = self.T * self.cin * self.cout
        body = rep.fetch(name, self.dest)
        what = "%s (%dx%d %d->%d %s)" % (name, int(np.sqrt(self.T)), int(np.sqrt(self.T)), self.cin, self.cout, self.kind)
        if self.kind == "mfma":
            wt, wd = mfma_rows(W)
            rep.single16(what + " wt", bits_of(body, 0, E, 2), wt.ravel(), self.inv32, self.sig64)
            rep.single16(what + " wd", bits_of(body, 2 * E, E, 2), wd.ravel(), self.inv32, self.sig64)
            if self.phase:
                W3 = self.w.astype(np.float64) / self.sig64
                for j, (S, A) in enumerate(phase_layouts(W3, 1 if self.pool else 0)):
                    rep.summed16("%s summed layout %d" % (what, j), bits_of(body, 4 * E + 32 * self.cin * self.cout * j, 16 * self.cin * self.cout, 2), S, A)
            for ctn, ss, fwd, bwd in self.frags:
                wt, wd = mfma_rows(W)
                rep.single16("%s fwd fragments" % what, rep.fetch(what + " fwd fragments", fwd).view(np.uint16), frag_encode(wt, ctn, ss),
                             self.inv32, self.sig64)
                rep.single16("%s bwd fragments" % what, rep.fetch(what + " bwd fragments", bwd).view(np.uint16), frag_encode(wd, ctn, ss),
                             self.inv32, self.sig64)
            return
        rep.single32(what + " fp32 copy", bits_of(body, 0, E, 4), self.w.ravel(), self.inv32, self.sig64)
        if self.kind != "plain":
            src = image_end_layout(W, CIN_SMALL_SIDE if self.kind == "img1" else COUT_SMALL_SIDE)
            rep.single16(what + " image-end layout", bits_of(body, self.img_off, self.img_elems, 2), src, self.inv32, self.sig64)


class Embed:
    def __init__(self, L, rs, v=10, e_dim=700, d=130, with_sigma=True, with_bias=True):
        self.table = (rs.randn(v, e_dim) * 0.1).astype(np.float32)
        self.w_e = (rs.randn(e_dim, d) * 0.2).astype(np.float32)
        self.b_e = (rs.randn(d) * 0.1).astype(np.float32) if with_bias else None
        self.sig = 0.7 if with_sigma else None
        self.keep = [torch.from_numpy(a).cuda() for a in (self.table, self.w_e)]
        self.keep += [torch.from_numpy(self.b_e).cuda() if with_bias else None,
                      torch.tensor([0.7], dtype=torch.float32).cuda() if with_sigma else None]
        self.dest = Dest(v * d * 4, [(0, v * d * 4)])
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.desc = L.EmbedDesc(v, e_dim, d, ptr(self.keep[0]), ptr(self.keep[1]), ptr(self.keep[3]), ptr(self.keep[2]), self.dest.ptr)
        self.shape = (v, d)

    def check(self, rep):
        got = rep.fetch("label embeddings", self.dest).view(np.uint32)
        if not rep.sentinels("label embeddings E", got):
            return
        sig = np.float64(np.float32(self.sig)) if self.sig else 1.0
        ref = self.table.astype(np.float64) @ (self.w_e.astype(np.float64) / sig) + (self.b_e if self.b_e is not None else 0.0)
        err = np.abs(got.view(np.float32).reshape(self.shape) - ref).max() / np.abs(ref).max()
        if err > EMBED_TOL:
            rep.errs.append("label embeddings E: max err %.3e of max|ref| (> %g)" % (err, EMBED_TOL))


class StepInputs:
    """The critic step's input rider: n images, their pooled halves and a zero-fill of fill_count floats."""
    LO, HI, SEED, STATE0 = 0.0, 1.0 / 128, 0x1234_5678_9ABC, 4242

    def __init__(self, L, ctx, mode, rs, n=3, fill_count=4 * 1037):
        self.L, self.mode, self.n, self.fill_count = L, mode, n, fill_count
        self.esz = 4 if mode == "f32" else 2
        self.images = rs.randint(0, 256, size=(n, 3, 32, 32)).astype(np.int32)
        fakes = rs.uniform(-1, 1, size=(n, 32, 32, 3)).astype(np.float32)
        self.fakes = fakes.view(np.uint32) if mode == "f32" else round16_bits(mode, fakes)
        self.img_dev = torch.from_numpy(self.images).cuda()
        self.state = torch.tensor([self.STATE0, 0], dtype=torch.int64).cuda()
        self.dtype = ctx.act_dtype

    def launch_args(self):
        """Fresh destinations, the stream reset to STATE0; returns the descriptor."""
        half = self.n * 3072 * self.esz
        self.x = Dest(2 * half, [(0, half)], init=[(half, self.fakes)])
        self.pooled = Dest(2 * self.n * 768 * self.esz, [(0, 2 * self.n * 768 * self.esz)])
        self.fill = Dest(self.fill_count * 4, [(0, self.fill_count * 4)])
        self.state.fill_(self.STATE0)
        return self.L.StepInputsDesc(self.n, self.dtype, self.img_dev.data_ptr(), self.x.ptr, self.pooled.ptr, self.LO, self.HI, self.SEED,
                                     self.state.data_ptr(), self.fill.ptr, self.fill_count, None, None, 0)

    def results(self, rep, tag):
        u = np.uint16 if self.esz == 2 else np.uint32
        x = rep.fetch(tag + " x", self.x)[:self.n * 3072 * self.esz].view(u)
        pooled = rep.fetch(tag + " pooled", self.pooled).view(u)
        fill = rep.fetch(tag + " fill", self.fill).view(np.uint32)
        return x, pooled, fill, int(self.state[0].item())

    def decode(self, bits):
        return bits.view(np.float32).astype(np.float64) if self.esz == 4 else decode16(self.mode, bits)

    def check(self, rep, got, ref):
        x, pooled, fill, state = got
        ok = rep.sentinels("step inputs x (real half)", x) & rep.sentinels("step inputs pooled", pooled)
        if (fill != 0).any():
            rep.errs.append("step inputs fill: %d of %d floats not zero" % (int((fill != 0).sum()), fill.size))
        adv = state - self.STATE0
        if adv != self.n * 3072 // 4:
            rep.errs.append("random stream moved on by %d quads, want n*3072/4 = %d" % (adv, self.n * 3072 // 4))
        if not ok:
            return
        if not (np.array_equal(x, ref[0]) and np.array_equal(pooled, ref[1])):
            rep.errs.append("step inputs differ from the same rider in a 1-item launch: x %d, pooled %d elements"
                            % (int((x != ref[0]).sum()), int((pooled != ref[1]).sum())))
        # x = 2 (img / 256 - .5) + noise, noise in [lo, hi), stored once: within half a storage ulp of that interval
        xs = self.decode(x).reshape(self.n, 32, 32, 3)
        pre = 2.0 * (self.images.transpose(0, 2, 3, 1) / 256.0 - 0.5)
        half_ulp = 0.5 * (np.spacing(np.abs(xs).astype(np.float32)).astype(np.float64) if self.esz == 4 else ulp16(self.mode, xs))
        noise = xs - pre
        if (noise < self.LO - half_ulp).any() or (noise > self.HI + half_ulp).any():
            rep.errs.append("step inputs x: noise outside [%g, %g): min %r max %r" % (self.LO, self.HI, noise.min(), noise.max()))
        # the 2x2 mean pool of the stored images, real then fake half: ((p00 + p10) + p01) + p11, x 0.25, in fp32
        allx = np.concatenate([xs, self.decode(self.fakes).reshape(self.n, 32, 32, 3)]).astype(np.float32)
        s = ((allx[:, 0::2, 0::2] + allx[:, 1::2, 0::2]) + allx[:, 0::2, 1::2]) + allx[:, 1::2, 1::2]
        s = (s * np.float32(0.25)).astype(np.float32)
        want = s.view(np.uint32).ravel() if self.esz == 4 else round16_bits(self.mode, s).ravel()
        if not np.array_equal(pooled, want):
            rep.errs.append("step inputs pooled: %d elements differ from the fp32 pool of the stored pixels" % int((pooled != want).sum()))


# ---------------------------------------------------------------------------------------------------------- launches
def launch(ctx, L, items, frags=(), embed=None, inputs=None):
    """One call of the ABI: rcgan_conv_prepare_batch without riders or fragment copies, else rcgan_conv_prepare_batch_frags.
    frags: [(item index, (ctn, ss, fwd Dest, bwd Dest))].  Returns the error code."""
    arr = (L.PrepareItem * max(len(items), 1))(*[it.prepare_item(L) for it in items])
    torch.cuda.synchronize()
    if not frags and embed is None and inputs is None:
        return ctx.lib.rcgan_conv_prepare_batch(ctx.h, arr, len(items))
    fa = (L.FragItem * max(len(frags), 1))(*[L.FragItem(i, ctn, ss, fw.ptr, bw.ptr) for i, (ctn, ss, fw, bw) in frags])
    return ctx.lib.rcgan_conv_prepare_batch_frags(ctx.h, arr, len(items), C.byref(embed) if embed is not None else None,
                                                  C.byref(inputs) if inputs is not None else None, fa, len(frags))


def run_case(ctx, mode, items, frags=(), embed=None, inputs=None):
    """Launch, then check every output of every item, the fragment copies and the riders against numpy."""
    from rcgan_amd import _lib as L
    ref = None
    if inputs is not None:       # the same rider in a 1-item launch first (its own destinations, the stream from STATE0)
        one = Item(L, ctx, mode, np.random.RandomState(1), (5, 7, 1, 8, 0, "plain"), True)
        ctx.check(launch(ctx, L, [one], inputs=inputs.launch_args()))
        ctx.sync()
        rep0 = Report(mode)
        ref = inputs.results(rep0, "1-item launch")
        rep0.done()
    si = inputs.launch_args() if inputs is not None else None
    ctx.check(launch(ctx, L, items, [(i, f) for i, f in frags], embed.desc if embed is not None else None, si))
    ctx.sync()
    rep = Report(mode)
    for i, it in enumerate(items):
        it.check(rep, "item %d" % i)
    if embed is not None:
        embed.check(rep)
    if inputs is not None:
        inputs.check(rep, inputs.results(rep, "step inputs"), ref)
    rep.done()


# the shapes: matrix-core ("mfma"), image-end ("img1": cin small, "img2": cout small) and plain items
def _specs(L):
    UP, POOL, DIRECT = L.CONV_IN_UPSAMPLE2X, L.CONV_OUT_MEANPOOL2, L.CONV_FORCE_DIRECT
    small = [(64, 64, 3, 8, 0, "mfma"), (5, 7, 1, 8, 0, "plain"), (3, 128, 1, 32, 0, "img1"), (128, 64, 1, 8, 0, "mfma"),
             (3, 10, 3, 8, 0, "plain"), (64, 128, 3, 8, 0, "mfma"), (64, 64, 3, 8, DIRECT, "plain"), (128, 3, 3, 32, 0, "img2")]
    big = [(512, 512, 3, 8, 0, "mfma"),          # 576 tiles: more than the 512 workgroups of a row
           (70, 250, 3, 8, 0, "plain"),          # 157500 elements: more than 512 workgroups x 256
           (1024, 256, 3, 8, UP, "mfma"),        # 2048 phase units: more than 1024 workgroups
           (3, 128, 3, 32, 0, "img1"), (3, 128, 1, 32, 0, "img1"), (128, 3, 3, 32, 0, "img2"),
           (128, 128, 3, 8, POOL, "mfma"), (64, 64, 1, 8, 0, "mfma"), (300, 1, 1, 8, 0, "plain"), (33, 65, 3, 8, 0, "plain")]
    phase = [(64, 64, 3, 8, UP, "mfma"), (64, 128, 3, 8, POOL, "mfma"), (128, 64, 3, 8, UP, "mfma"), (128, 128, 3, 8, POOL, "mfma")]
    return small, big, phase


FRAG_LAYOUTS = [(4, 18), (2, 9), (1, 18), (4, 6)]     # (ctn, ss) the 64-channel filters take; 128 -> 128 also takes (2, 36)


@pytest.mark.parametrize("n", [1, 47, 48, 49, 97])
def test_item_counts_and_launch_boundaries(dev, n):
    """n items over one, two or three launches (48 per launch).  Both riders ride in the first launch only (the random stream moves
    on once); fragment copies of items 0, 47, 48 and 96 land in the launch that prepares their item."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(100 + n)
    small, _, _ = _specs(L)
    frag_items = [i for i in (0, 47, 48, 96) if i < n] if mode != "f32" else []
    items = [Item(L, ctx, mode, rs, small[0] if i in frag_items else small[i % len(small)], i % 3 != 1) for i in range(n)]
    frags = [(i, items[i].add_frag(L, *FRAG_LAYOUTS[j % len(FRAG_LAYOUTS)])) for j, i in enumerate(frag_items)]
    embed = Embed(L, rs, with_sigma=n % 2 == 1, with_bias=n % 2 == 1)
    run_case(ctx, mode, items, frags, embed, StepInputs(L, ctx, mode, rs))


def test_item_kinds_in_one_launch(dev):
    """Matrix-core, image-end and plain items in one rcgan_conv_prepare_batch, with the stride loops of each row kind: a 3x3 512 -> 512
    filter (576 tiles), a 3x3 70 -> 250 plain filter (157500 elements) and an upsample 1024 -> 256 filter (2048 phase units)."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(7)
    _, big, _ = _specs(L)
    items = [Item(L, ctx, mode, rs, s, i % 2 == 0) for i, s in enumerate(big)]
    run_case(ctx, mode, items)


@pytest.mark.parametrize("nphase", [8, 9])
def test_phase_filters_ride_and_fall_back(dev, nphase):
    """8 summed phase filters ride in the launch; a 9th takes conv_prepare_phase_launch behind it.  Both families, sigma or not."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    if mode == "f32":
        pytest.skip("summed phase filters exist for 16-bit matrix-core items only")
    rs = np.random.RandomState(20 + nphase)
    small, _, phase = _specs(L)
    items = []
    for i in range(nphase):
        items.append(Item(L, ctx, mode, rs, phase[i % len(phase)], i % 3 != 2))
        if i % 4 == 1:
            items.append(Item(L, ctx, mode, rs, small[i % len(small)], True))
    assert sum(it.phase for it in items) == nphase
    run_case(ctx, mode, items)


def test_rows_past_63(dev):
    """The largest launch the ABI admits: 48 items, 8 of them with summed phase filters, 12 fragment copies and both riders --
    48 + 8 + 12 + 2 = 70 rows of conv_prepare_batch_kernel's grid.  The row lookup has to reach every one of them: the last
    fragment copies, the label embeddings and the step inputs sit in rows 64-69."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    if mode == "f32":
        pytest.skip("phase filters and fragment copies need matrix-core (16-bit) items: an f32 launch cannot reach 64 rows")
    rs = np.random.RandomState(63)
    small, _, phase = _specs(L)
    specs = []
    for i in range(MAX_ITEMS):
        if i % 6 == 5:
            specs.append(phase[(i // 6) % len(phase)])        # items 5, 11, ..., 47: 8 phase filters
        else:
            specs.append(small[i % len(small)])
    items = [Item(L, ctx, mode, rs, s, i % 4 != 3) for i, s in enumerate(specs)]
    assert sum(it.phase for it in items) == MAX_PHASE_RIDE
    # 12 fragment copies: 3x3 matrix-core items, the phase filters among them, the last one on the last item
    cands = [i for i, it in enumerate(items) if it.kind == "mfma" and it.T == 9]
    frag_items = cands[:MAX_FRAGS - 1] + [MAX_ITEMS - 1]
    assert len(set(frag_items)) == MAX_FRAGS
    frags = [(i, items[i].add_frag(L, *FRAG_LAYOUTS[j % len(FRAG_LAYOUTS)])) for j, i in enumerate(frag_items)]
    run_case(ctx, mode, items, frags, Embed(L, rs), StepInputs(L, ctx, mode, rs))


def test_rejections_launch_nothing(dev):
    """Arguments rcgan_conv_prepare_batch_frags refuses: an error naming the problem, and no destination or stream touched."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    rs = np.random.RandomState(3)
    items = [Item(L, ctx, mode, rs, s, True) for s in [(64, 64, 3, 8, 0, "mfma"), (5, 7, 1, 8, 0, "plain"), (128, 64, 1, 8, 0, "mfma")]]
    fd = items[0].add_frag(L, 4, 18)
    ctn, ss, fw, bw = fd
    embed = Embed(L, rs)
    inputs = StepInputs(L, ctx, mode, rs)
    si = inputs.launch_args()
    bad_fill = inputs.L.StepInputsDesc(*[getattr(si, f) for f, _ in si._fields_])
    bad_fill.fill_count = si.fill_count - 1
    big_v = L.EmbedDesc(*[getattr(embed.desc, f) for f, _ in embed.desc._fields_])
    big_v.v = 17

    def frag(i, c=ctn, s=ss, f=fw, b=bw):
        return (i, (c, s, f, b))

    null = type("N", (), {"ptr": None})()
    cases = [
        ("13 fragment copies", dict(items=items, frags=[frag(0)] * (MAX_FRAGS + 1)), "at most 12"),
        ("fragment item past the items", dict(items=items, frags=[frag(3)]), "bad item"),
        ("negative fragment item", dict(items=items, frags=[frag(-1)]), "bad item"),
        ("null fragment destination", dict(items=items, frags=[frag(0, b=null)]), "null destination"),
        ("fragment copy of a 1x1 filter", dict(items=items, frags=[frag(2)]), "not a 16-bit 3x3 filter"),
        ("fragment copy of a plain filter", dict(items=items, frags=[frag(1)]), "not a 16-bit 3x3 filter"),
        ("fragment tiles that do not divide the channels", dict(items=items, frags=[frag(0, c=8)]), "not a 16-bit 3x3 filter"),
        ("fragment steps that do not divide the reduction", dict(items=items, frags=[frag(0, s=36)]), "not a 16-bit 3x3 filter"),
        ("label embeddings with 0 items", dict(items=[], embed=embed.desc), "at least one filter"),
        ("step inputs with 0 items", dict(items=[], inputs=si), "at least one filter"),
        ("fragment copies with 0 items", dict(items=[], frags=[frag(0)]), "at least one filter"),
        ("more than 16 label rows", dict(items=items, embed=big_v), "bad embed desc"),
        ("a fill that is not whole float4", dict(items=items, inputs=bad_fill), "whole float4"),
    ]
    for what, kw, msg in cases:
        rc = launch(ctx, L, **kw)
        err = ctx.lib.rcgan_last_error(ctx.h).decode()
        assert rc == L.EINVALID_ARG, (what, rc, err)
        assert msg in err, (what, err)
    ctx.sync()
    rep = Report(mode)
    dests = [("item %d" % i, it.dest) for i, it in enumerate(items)]
    for what, d in dests + [("fwd fragments", fw), ("bwd fragments", bw), ("E", embed.dest), ("x", inputs.x), ("pooled", inputs.pooled),
                            ("fill", inputs.fill)]:
        body = rep.fetch(what, d)
        for off, n in d.outs:
            if (body[off:off + n] != SENTINEL).any():
                rep.errs.append("%s written by a rejected call" % what)
    assert int(inputs.state[0].item()) == StepInputs.STATE0, "a rejected call moved the random stream on"
    rep.done()
