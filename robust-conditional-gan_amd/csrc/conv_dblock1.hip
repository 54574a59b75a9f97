// D.Block.1 of the CIFAR discriminator, the 32x32x3 -> 16x16x128 input block (gan_resnet.py:331-353, OptimizedResBlockDisc1), FORWARD, as
// ONE launch:
//     h  = 16bit(Conv1(x) + b1)                            3x3, 3 -> 128, on 32 x 32 pixels, no ReLU on x          -> HBM
//     xp = 16bit(meanpool2(x))                             (((x00 + x10) + x01) + x11) / 4, as meanpool2_fwd_kernel / the input riders
//     t  = 16bit(Shortcut(xp) + bs)                        1x1, 3 -> 128
//     y  = 16bit(t + meanpool2(Conv2(relu(h))) + b2)       as one 4x4 stride-2 convolution with the summed filters (x 1/4), K = 16 * 128
// Why.  As three launches (conv_img_small_red_kernel twice, the gather-form 64 x 64 tile kernel) the block costs about 50 us at n = 128: h
// (33.5 MB) is written by one launch and read back by the next, two launches start 512 workgroups of almost no arithmetic, and each of
// the 1024 tiles of Conv2 re-fetches a 256 KB filter slice.  Same construction as conv_dblock2.hip: there is no norm layer in D, so
//   * workgroup (image, band b) owns 8 rows of h and 4 pooled rows, all 128 channels.  Pooled rows 4b .. 4b + 3 need rows 8b - 1 .. 8b + 8
//     of h, which need rows 8b - 2 .. 8b + 9 of x: the workgroup computes 10 rows of h (25 % more Conv1: 160 MFMAs in all) and stores the 8
//     it owns.  Nothing is exchanged between workgroups, exactly one workgroup writes each element;
//   * stage 1 is conv_img_small_red_kernel's arithmetic: one 16x16x32 MFMA per 16 pixels and 16 channels over the [128][32] filter rows
//     conv_image.hip prepares (k = tap * 3 + c, read straight from the prepared buffer: 16 rows of one fragment are one contiguous KiB
//     already), C = 0, + bias in fp32, one rounding.  Its im2col columns come from a zero-framed 12 x 34 x 3 patch in LDS.  h goes to HBM
//     (the backward pass reads it) and relu(h) of all 10 rows stays in LDS as a zero-framed 10 x 34 image of 256-byte pixels;
//   * stage 2: a wavefront owns 32 output channels x the 64 pooled pixels; 64 K-steps of the summed filters over relu(h), one accumulator
//     per tile, K-tiles in order (conv_mfma_glds_kernel<64, 64, 2, 1, 2>: KS = 1).  The filters stream through a ring of 32 K-steps in the
//     256 AccVGPRs (2 KiB per wavefront and K-step); its first lap is requested BEFORE stage 1, which uses no AccVGPR, so the stream's L2
//     round trip hides behind Conv1.  The shortcut is one more MFMA per tile in the epilogue, over xp formed in LDS from the patch.
// Rounding points and reduction orders are the three launches': every output has their bits.
#include "conv_mfma.h"
#include "mfma_util.h"
#include "rf_asm.h"

namespace {

constexpr int D1_PW = 34;                                  // padded row: 32 pixels + two halo columns
constexpr int D1_XROWS = 12;                               // input patch: image rows 8b - 2 .. 8b + 9
constexpr int D1_XELEMS = D1_XROWS * D1_PW * 3;            // 16-bit elements of the patch; element D1_XELEMS is a zero (im2col columns k >= 27)
constexpr int D1_XBYTES = (D1_XELEMS * 2 + 16 + 255) / 256 * 256;
constexpr int D1_HROWS = 10;                               // relu(h): rows 8b - 1 .. 8b + 8
constexpr int D1_HNPP = D1_HROWS * D1_PW;
constexpr int D1_HBYTES = D1_HNPP * 256;
constexpr int D1_XPBYTES = 64 * 4 * 2;                     // the 4 x 16 pooled input pixels, (c0, c1, c2, 0) each
constexpr int D1_BIAS = 3 * 128 * 4;
constexpr int D1_LDS = D1_XBYTES + D1_HBYTES + D1_XPBYTES + D1_BIAS;
constexpr int D1_RING = 32;                                // stage 2: K-steps in flight
constexpr int D1_STEPS2 = 64;                              // stage 2: 16 taps x 4 channel quarters
static_assert(D1_LDS <= 160 * 1024, "LDS of one CU");
static_assert(D1_STEPS2 % D1_RING == 0 && D1_RING * 8 == 256, "the ring is the 256 AccVGPRs");

struct Db1Args {
  const bf16_t* x;         // [n][32][32][3]
  const bf16_t* wk1;       // Conv1: [128][32] rows of conv_image.hip (k = tap * 3 + c)
  const bf16_t* wks;       // Shortcut: [128][32] rows (k = c)
  const bf16_t* w2;        // Conv2 (summed, gather layout) fragments (rf_asm.h: dblock1_frag_items)
  const float *b1, *b2, *bs;
  bf16_t *h, *xp, *y;      // [n][32][32][128], [n][16][16][3] or null (the caller has the pooled images already), [n][16][16][128]
  unsigned long long* stamps;   // diagnostics (rcgan_debug_stamps): 16 s_memtime stamps per workgroup, normally null
};

__global__ __launch_bounds__(256) void conv_dblock1_kernel(Db1Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, kc = lane >> 4;
  const int n = (int)blockIdx.x >> 2, band = (int)blockIdx.x & 3;
  bf16_t* const xs = (bf16_t*)smem;
  unsigned char* const himg = smem + D1_XBYTES;
  bf16_t* const xps = (bf16_t*)(himg + D1_HBYTES);
  float* const bias_s = (float*)(himg + D1_HBYTES + D1_XPBYTES);       // b1, b2, bs
  auto stamp = [&](int k) __attribute__((always_inline)) {
    if (a.stamps && tid == 0) a.stamps[(long)blockIdx.x * 16 + k] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);

  // ---- the input patch: 12 x 34 pixels x 3 channels, zero outside the image (the tensor is 6 KB per image and lives in L2) ----
  const bf16_t* const img = a.x + (long)n * (32 * 32 * 3);
  for (int e = tid; e < D1_XELEMS + 8; e += 256) {
    bf16_t v = 0;
    if (e < D1_XELEMS) {
      const int pr = e / (D1_PW * 3), rem = e - pr * (D1_PW * 3), pc = rem / 3, c = rem - pc * 3;
      const int ih = 8 * band - 2 + pr, iw = pc - 1;
      if (ih >= 0 && ih < 32 && iw >= 0 && iw < 32) v = img[(ih * 32 + iw) * 3 + c];
    }
    xs[e] = v;
  }
  if (tid < 96) *(float4*)(bias_s + tid * 4) = *(const float4*)((tid < 32 ? a.b1 : tid < 64 ? a.b2 : a.bs) + (tid & 31) * 4);
  // Conv1's filter fragments.  Row j of fragment pair (2q, 2q + 1) is channel q * 32 + (j >> 2) * 8 + (i & 1) * 4 + (j & 3), so that D rows
  // 4 kc .. 4 kc + 3 of the pair are channels q * 32 + kc * 8 + 0 .. 7 of the lane's pixel: one 16-byte store (conv_img_small_red_kernel)
  bf16x8_t wf[8], wsf[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ch = (i >> 1) * 32 + (r >> 2) * 8 + (i & 1) * 4 + (r & 3);
    wf[i] = *(const bf16x8_t*)(a.wk1 + ch * 32 + kc * 8);
  }
  // the shortcut's, in stage 2's layout: fragment ct = channels wave * 32 + ct * 16 + (row)
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) wsf[ct] = *(const bf16x8_t*)(a.wks + (wave * 32 + ct * 16 + r) * 32 + kc * 8);
  // the zero frame of relu(h): columns 0 and 33 of every row; the row above the image (band 0) / below it (band 3).  Stage 1 writes the rest.
  for (int i = tid; i < 2 * D1_HROWS * 16; i += 256) {
    const int p = i >> 4, pp = (p >> 1) * D1_PW + (p & 1) * (D1_PW - 1);
    ((uint4*)(himg + pp * 256))[i & 15] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (band == 0 || band == 3) {
    uint4* const row = (uint4*)(himg + (band ? (D1_HROWS - 1) * D1_PW * 256 : 0));
    for (int i = tid; i < D1_PW * 16; i += 256) row[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  // (every load above has landed before the filter stream below is requested: the compiler waits for its own loads without knowing the
  // asm-issued ones, which it would then wait for as well)
#pragma unroll
  for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(wf[i]));
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) asm volatile("" : "+v"(wsf[ct]));
  stamp(1);

  // ---- stage 2's filters: K-step u into ring slot u % D1_RING = WA[slot / 2][2 * (slot & 1) + channel tile]; the first lap goes out now ----
  i32x4_t WA[D1_RING / 2][4];
  const bf16_t* const w2c = a.w2 + (long)wave * (D1_STEPS2 * 1024) + lane * 8;      // K-step u: + u * 1024
  rf_for<0, D1_RING>([&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value;
    rf_load_a<0>(WA[u >> 1][2 * (u & 1)], w2c + u * 1024); rf_load_a<1024>(WA[u >> 1][2 * (u & 1) + 1], w2c + u * 1024);
  });
  auto w2load = [&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = u % D1_RING;
    const bf16_t* const p = w2c + u * 1024;
    rf_load_a_inplace<0>(WA[slot >> 1][2 * (slot & 1)], p); rf_load_a_inplace<1024>(WA[slot >> 1][2 * (slot & 1) + 1], p);
  };

  // ---- xp: the 2x2 mean of the patch, fp32 from the stored 16-bit values, rounded once; thread = one channel of a pooled pixel ----
  if (tid < 192) {
    const int p = tid / 3, c = tid - p * 3, pi = p >> 4, pj = p & 15;
    const int e00 = ((2 + 2 * pi) * D1_PW + 1 + 2 * pj) * 3 + c;         // image pixel (8 band + 2 pi, 2 pj)
    const float v = (((bf16_to_f32(xs[e00]) + bf16_to_f32(xs[e00 + D1_PW * 3])) + bf16_to_f32(xs[e00 + 3])) + bf16_to_f32(xs[e00 + D1_PW * 3 + 3])) * 0.25f;
    const bf16_t o = f32_to_bf16(v);
    xps[p * 4 + c] = o;
    if (a.xp) a.xp[(((long)n * 16 + 4 * band + pi) * 16 + pj) * 3 + c] = o;
  } else {
    xps[(tid - 192) * 4 + 3] = 0;
  }

  // ---- stage 1: wavefront w takes the 16-pixel tiles w, w + 4, .. of the 10 x 32 pixels of h (tile t: row t / 2, columns (t & 1) * 16 ..) ----
  int koff[8];                                   // patch element of im2col column k = kc * 8 + e, relative to the output pixel; -1: k >= 27
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = kc * 8 + e, tap = k / 3, c = k - tap * 3, kh = tap / 3, kw = tap - kh * 3;
    koff[e] = k < 27 ? (kh * D1_PW + kw) * 3 + c : -1;
  }
  for (int t = wave; t < 2 * D1_HROWS; t += 4) {
    const int hr = t >> 1, col = (t & 1) * 16 + r;
    const int ih = 8 * band - 1 + hr;            // image row of h
    if (ih < 0 || ih >= 32) continue;            // (wavefront-uniform) no such row: the zero frame stands for it
    const int base = (hr * D1_PW + col) * 3;     // patch pixel (hr, col) = input pixel (ih - 1, col - 1): tap (0, 0)
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = xs[koff[e] >= 0 ? base + koff[e] : D1_XELEMS];
    const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)));
    const int pp = hr * D1_PW + col + 1;
    const bool own = hr >= 1 && hr <= 8;
    bf16_t* const orow = a.h + (((long)n * 32 + ih) * 32 + col) * 128 + kc * 8;
    // (asm MFMAs on VGPRs, C = 0: the AccVGPRs belong to the stream in flight; the compiler's hazard recogniser does not see them, so the
    // waits around them are placed by hand)
    f32x4_t lo[4], hi[4];
    asm volatile("s_nop 1" ::: "memory");
#pragma unroll
    for (int q = 0; q < 4; ++q) { rf_mfma_vv0(lo[q], wf[2 * q], xf); rf_mfma_vv0(hi[q], wf[2 * q + 1], xf); }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 ba = *(const float4*)(bias_s + q * 32 + kc * 8), bb = *(const float4*)(bias_s + q * 32 + kc * 8 + 4);
      uint4 pk;
      pk.x = pack_h16x2(lo[q][0] + ba.x, lo[q][1] + ba.y);
      pk.y = pack_h16x2(lo[q][2] + ba.z, lo[q][3] + ba.w);
      pk.z = pack_h16x2(hi[q][0] + bb.x, hi[q][1] + bb.y);
      pk.w = pack_h16x2(hi[q][2] + bb.z, hi[q][3] + bb.w);
      if (own) *(uint4*)(orow + q * 32) = pk;
      pk.x = relu_bf16x2(pk.x); pk.y = relu_bf16x2(pk.y); pk.z = relu_bf16x2(pk.z); pk.w = relu_bf16x2(pk.w);
      // 16-byte slots XOR-swizzled with (pixel / 2) & 15: stage 2 reads pixels two apart
      *(uint4*)(himg + pp * 256 + (((q * 4 + kc) ^ ((pp >> 1) & 15)) << 4)) = pk;
    }
  }
  stamp(2);
  // the h stores and the first lap have landed (stores and loads retire in order only among themselves: from here on only loads are counted)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  rf_barrier();                                  // relu(h) and xp are complete
  stamp(3);

  // ---- stage 2: this wavefront's 32 channels x the 64 pooled pixels; pixel tile pt = pooled row 4 band + pt, lane's pixel = column r ----
  int rr = r;
  asm volatile("" : "+v"(rr));                   // (opaque: the 256 fragment addresses must not be hoisted and spilled)
  auto xread = [&](auto ic, bf16x8_t (&xf)[4]) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, tap = u >> 2, cq = u & 3, uu = tap >> 2, vv = tap & 3;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {             // tap (uu, vv) of the 4x4 stride-2 window: h pixel (2 i + uu - 1, 2 j + vv - 1)
      const int pp = (2 * pt + uu) * D1_PW + vv + 2 * rr;
      xf[pt] = *(const bf16x8_t*)(himg + pp * 256 + (((cq * 4 + kc) ^ ((pp >> 1) & 15)) << 4));
    }
  };
  f32x4_t acc2[4][2];                            // [pixel tile][channel tile]
  bf16x8_t xf2[2][4];
  xread(std::integral_constant<int, 0>{}, xf2[0]);
  rf_for<0, D1_STEPS2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = u % D1_RING;
    if constexpr (u + 1 < D1_STEPS2) xread(std::integral_constant<int, u + 1>{}, xf2[(u + 1) & 1]);
    // loads retire in order: K-step u has landed once at most the loads of the K-steps behind it (u + 1 .. u + D1_RING - 1) are outstanding
    rf_wait<2 * ((u + D1_RING - 1 < D1_STEPS2 - 1 ? u + D1_RING - 1 : D1_STEPS2 - 1) - u)>();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const i32x4_t& w = WA[slot >> 1][2 * (slot & 1) + ct];
        if constexpr (u == 0) rf_mfma_a0e(acc2[pt][ct], w, xf2[u & 1][pt]);
        else rf_mfma_a(acc2[pt][ct], w, xf2[u & 1][pt]);
      }
    if constexpr (u + D1_RING < D1_STEPS2) w2load(std::integral_constant<int, u + D1_RING>{});
  });
  stamp(4);
  // (MFMA results read by non-MFMA instructions: the asm MFMAs are invisible to the compiler's hazard recogniser)
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  // ---- epilogue: t = 16bit(Shortcut(xp) + bs), one MFMA per tile with C = 0;  y = 16bit((Conv2 + b2) + t) ----
  f32x4_t accs[4][2];
  bf16x8_t xpf[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const uint2 xv = *(const uint2*)(xps + (pt * 16 + r) * 4);
    xpf[pt] = __builtin_bit_cast(bf16x8_t, kc == 0 ? make_uint4(xv.x, xv.y, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u));
    asm volatile("" : "+v"(xpf[pt]));
  }
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) rf_mfma_vv0(accs[pt][ct], wsf[ct], xpf[pt]);
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const f32x4_t s = accs[pt][ct];
      const int c0 = wave * 32 + ct * 16 + 4 * kc;
      const float4 b2 = *(const float4*)(bias_s + 128 + c0), bs = *(const float4*)(bias_s + 256 + c0);
      uint2 t;
      t.x = pack_h16x2(s[0] + bs.x, s[1] + bs.y);
      t.y = pack_h16x2(s[2] + bs.z, s[3] + bs.w);
      const f32x4_t c2 = acc2[pt][ct];
      uint2 pk;
      pk.x = pack_h16x2((c2[0] + b2.x) + h16_lo(t.x), (c2[1] + b2.y) + h16_hi(t.x));
      pk.y = pack_h16x2((c2[2] + b2.z) + h16_lo(t.y), (c2[3] + b2.w) + h16_hi(t.y));
      *(uint2*)(a.y + (((long)n * 16 + 4 * band + pt) * 16 + r) * 128 + c0) = pk;
    }
  }
  if (a.stamps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp(5);
  }
}

bool dblock1_takes(const rcgan_conv_desc* d) {
  if (!d || d->dtype != RCGAN_H16 || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->flags != 0) return false;
  if (!(d->n >= 1 && d->h == 32 && d->w == 32 && d->cin == 3 && d->cout == 128)) return false;
  return (long)d->n * d->h * d->w * d->cout < (1L << 31);
}

}  // namespace

extern "C" {

// d: D.Block.1.Conv1's descriptor (n x 32 x 32 x 3 -> 128, 3x3, no flags, the build's 16-bit dtype); dblock1_frag: what
// rcgan_fragments_prepare_dblocks wrote for the current weights.
int rcgan_dblock1_ok(const rcgan_conv_desc* d, const void* dblock1_frag) { return dblock1_takes(d) && dblock1_frag ? 1 : 0; }

size_t rcgan_dblock1_fragment_bytes(void) { return (size_t)DB1_FRAG_ELEMS * sizeof(bf16_t); }

// conv1_prepared / shortcut_prepared: rcgan_conv_prepare's buffers of Conv1 (d) and of the 1x1 shortcut (n x 16 x 16 x 3 -> 128): their
// image-end rows are read in place.  h [n][32][32][128] and y [n][16][16][128] are written; xp [n][16][16][3] too unless it is NULL (the
// caller holds the pooled images already): everything the block's (unfused) backward pass reads.
int rcgan_dblock1_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* conv1_prepared, const void* shortcut_prepared,
                      const void* dblock1_frag, const float* bias1, const float* bias2, const float* bias_shortcut, void* h, void* xp, void* y) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, rcgan_dblock1_ok(d, dblock1_frag), "not the 32x32x3 input block / missing fragment copy (rcgan_dblock1_ok)");
  RC_REQUIRE(ctx, x && conv1_prepared && shortcut_prepared && bias1 && bias2 && bias_shortcut && h && y, "null argument");
  const rcgan_conv_desc ds = {d->n, 16, 16, 3, 128, 1, 1, 1, d->dtype, 0};
  RC_REQUIRE(ctx, img_side(d) == 1 && img_side(&ds) == 1, "the image-end rows of Conv1 and the shortcut are not prepared for this build");
  Db1Args a;
  a.x = (const bf16_t*)x;
  a.wk1 = (const bf16_t*)((const char*)conv1_prepared + img_extra_offset(d));
  a.wks = (const bf16_t*)((const char*)shortcut_prepared + img_extra_offset(&ds));
  a.w2 = (const bf16_t*)dblock1_frag;
  a.b1 = bias1; a.b2 = bias2; a.bs = bias_shortcut;
  a.h = (bf16_t*)h; a.xp = (bf16_t*)xp; a.y = (bf16_t*)y;
  a.stamps = (unsigned long long*)ctx->dbg_stamps;
  static bool attr_set = false;
  if (!attr_set) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_dblock1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)D1_LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL(conv_dblock1_kernel, dim3(4 * d->n), dim3(256), D1_LDS, ctx->stream, a);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
