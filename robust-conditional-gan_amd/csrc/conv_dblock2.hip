// D.Block.2 of the CIFAR discriminator, the 16x16x128 -> 8x8x128 down block (gan_resnet.py:275-328 with resample='down', :396), FORWARD, as
// ONE launch:
//     h  = bf16(Conv1(relu(x)) + b1)                       3x3, 128 -> 128, on 16 x 16 pixels
//     xp = bf16(meanpool2(x))                              the shortcut's operand (its filter gradient reads it)
//     t  = bf16(Shortcut(xp) + bs)                         1x1
//     y  = bf16(t + meanpool2(Conv2(relu(h))) + b2)        as one 4x4 stride-2 convolution with the summed filters (x 1/4)
// Why.  As four launches (2x2 mean, 1x1 convolution, conv_rf_kernel, the gather-form tile kernel) the block costs 40 us for 14 GFLOP: every
// launch pays dispatch, a cold patch and filter fetch, pipeline fill and drain, and two of them start 256 workgroups of very little work.
// There is no norm layer in D, so an image never meets another image, and behind a 3x3 convolution the dependency cone of the 4x4 stride-2
// convolution is ONE halo row: pooled rows 0..3 need rows 0..8 of h, pooled rows 4..7 need rows 7..15.
//   * workgroup (image, half) owns 8 rows of h and 4 pooled rows, all 128 channels, and computes 9 rows of h (12.5 % more Conv1 work):
//     nothing is exchanged between workgroups, exactly one workgroup writes each element, the halo row of h stays in LDS;
//   * stage 1 is conv_rf_kernel<128, 16>'s arithmetic (conv_rf.hip: patch by LDS-DMA, the filter slice of a wavefront in registers, the
//     reduction split over two wavefronts whose partial tiles meet in LDS; p0 + p1 in fp32, + bias, one rounding): h is bit-identical.
//     Its nine pixel tiles run as two groups of four (the owned rows) and a last group of one (the halo row); the epilogue stores the
//     owned rows to HBM and leaves relu(h) of all nine in LDS as a zero-padded 10 x 18 image;
//   * stage 2: a wavefront owns 32 output channels x the 32 pooled pixels; 4 K-steps of the shortcut over xp (formed in LDS from the
//     patch BEFORE its in-place ReLU: (((x00 + x10) + x01) + x11) / 4 in fp32, as resample2_vec_kernel) and 64 K-steps of the summed
//     filters over relu(h).  No reduction split over wavefronts, so no second exchange.  The filters stream through the 256 AccVGPRs stage 1's filters
//     leave dead: a ring of 32 K-steps (2 KiB per wavefront each), whose first lap is issued by the LAST group of stage 1 behind the MFMAs
//     that consume each register for the last time, so the stream's L2 round trip hides behind the halo row and the exchange.
// Rounding points are the four launches': h, xp, t, y.  The fp32 reductions run in the four launches' order too (stage 2 keeps the even and
// the odd 64-deep K-tiles of Conv2 apart, as the two wavefront groups of the gather-form tile kernel do), so at the shapes those kernels
// take in the training step every output has their bits.
#include <type_traits>

#include "conv_mfma.h"
#include "mfma_util.h"
#include "rf_asm.h"

namespace {

constexpr int DB_PW = 18;                                  // padded row: 16 pixels + two halo columns
constexpr int DB_XNPP = 11 * DB_PW;                        // input patch: image rows r0 - 1 .. r0 + 9 of the 9 computed rows r0 .. r0 + 8
constexpr int DB_XBYTES = (DB_XNPP * 256 + 1023) / 1024 * 1024;
constexpr int DB_HNPP = 10 * DB_PW;                        // relu(h): the 9 computed rows and one zero row (above the image / below it)
constexpr int DB_HBYTES = DB_HNPP * 256;
constexpr int DB_XPBYTES = 32 * 256;                       // the 4 x 8 pooled input pixels
constexpr int DB_RED = 4 * 8 * 64 * 16;                    // partial-tile exchange: a wavefront sends the half of its tiles its partner finishes
constexpr int DB_BIAS = 3 * 128 * 4;
constexpr int DB_LDS = DB_XBYTES + DB_HBYTES + DB_XPBYTES + DB_RED + DB_BIAS;
constexpr int DB_UPFRONT = 4;                              // stage 1: K-steps of filters requested before the K loop (conv_rf.hip: RF_UPFRONT)
constexpr int DB_ASTEPS = 16;                              // stage 1: K-steps held in AccVGPRs; = half the stage 2 ring
constexpr int DB_RING = 32;                                // stage 2: K-steps in flight
constexpr int DB_STEPS2 = 4 + 64;                          // stage 2: shortcut K-steps, then Conv2's
static_assert(DB_LDS <= 160 * 1024, "LDS of one CU");
static_assert(DB_RING == 2 * DB_ASTEPS, "the ring is stage 1's AccVGPR block");

struct Db2Args {
  const bf16_t* x;         // [n][16][16][128]
  const bf16_t* w1;        // Conv1: forward fragments of rcgan_conv_rf_prepare
  const bf16_t* w2;        // Conv2 (summed, gather layout) + Shortcut fragments (rf_asm.h: dblock2_frag_items)
  const float *b1, *b2, *bs;
  bf16_t *h, *xp, *y;      // [n][16][16][128], [n][8][8][128], [n][8][8][128]
  const bf16_t* zero;      // >= 16 zero bytes (halo source)
  unsigned long long* stamps;   // diagnostics (rcgan_debug_stamps): 16 s_memtime stamps per workgroup, normally null
};

__global__ __launch_bounds__(256) void conv_dblock2_kernel(Db2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = wave & 1, cb = wave >> 1;                 // stage 1: K slice, 64-channel block
  const int r = lane & 15, kc = lane >> 4;
  const int n = (int)blockIdx.x >> 1, hf = (int)blockIdx.x & 1;
  const int xr0 = hf ? 6 : -1;                             // image row of patch row 0; computed row cr is image row 7 * hf + cr
  unsigned char* const himg = smem + DB_XBYTES;
  unsigned char* const xps = himg + DB_HBYTES;
  float4* const red = (float4*)(xps + DB_XPBYTES);
  float* const bias_s = (float*)(xps + DB_XPBYTES + DB_RED);     // b1, b2, bs
  auto stamp = [&](int k) __attribute__((always_inline)) {
    if (a.stamps && tid == 0) a.stamps[(long)blockIdx.x * 16 + k] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);

  i32x4_t WA[DB_ASTEPS][4], WV[18 - DB_ASTEPS][4];
  const bf16_t* const wl = a.w1 + ((long)(cb * 2 + kq) * 18) * (4 * 512) + lane * 8;
  const bf16_t* const w2l = a.w2 + DB2_FRAG_CONV2 + (long)wave * (4 * 1024) + lane * 8;      // stage 2, K-step u < 4: + u * 1024
  const bf16_t* const w2c = a.w2 + (long)wave * (64 * 1024) + lane * 8;                      // K-step u >= 4: + (u - 4) * 1024

  // ---- the input patch by LDS-DMA (conv_rf.hip): 11 x 18 pixels, 16-byte slots XOR-swizzled with the pixel index on the source side ----
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  constexpr int ninst = (DB_XNPP * 16 + 63) / 64;
  const bf16_t* const img = a.x + (long)n * 256 * 128;
#pragma unroll
  for (int i = 0; i < (ninst + 3) / 4; ++i) {
    const int q = i * 4 + wave;
    if (q < ninst) {                               // (wavefront-uniform)
      const int c = q * 64 + lane, pp = c >> 4, sp = c & 15;
      const int pr = pp / DB_PW, pc = pp - pr * DB_PW;
      const int ih = xr0 + pr, iw = pc - 1;
      const bool ok = pp < DB_XNPP && ih >= 0 && ih < 16 && iw >= 0 && iw < 16;
      const int off = ((ih * 16 + iw) * 128 + ((sp ^ (pp & 15)) << 3)) * 2;
      const char* src = ok ? (const char*)img + off : (const char*)a.zero;
      glds16_asm(src, lds0 + q * 1024);
    }
  }
  float4 bias_v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 96) bias_v = *(const float4*)((tid < 32 ? a.b1 : tid < 64 ? a.b2 : a.bs) + (tid & 31) * 4);
  auto wload = [&](auto ic) __attribute__((always_inline)) {
    constexpr int s = decltype(ic)::value;
    const bf16_t* const p = wl + s * (4 * 512);
    if constexpr (s < DB_ASTEPS) {
      rf_load_a<0>(WA[s][0], p); rf_load_a<1024>(WA[s][1], p); rf_load_a<2048>(WA[s][2], p); rf_load_a<3072>(WA[s][3], p);
    } else {
      rf_load_v<0>(WV[s - DB_ASTEPS][0], p); rf_load_v<1024>(WV[s - DB_ASTEPS][1], p);
      rf_load_v<2048>(WV[s - DB_ASTEPS][2], p); rf_load_v<3072>(WV[s - DB_ASTEPS][3], p);
    }
  };
  // stage 2's K-step u into ring slot u % DB_RING = WA[slot / 2][2 * (slot & 1) + channel tile]
  auto w2load = [&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = u % DB_RING;
    const bf16_t* const p = u < 4 ? w2l + u * 1024 : w2c + (u - 4) * 1024;
    rf_load_a_inplace<0>(WA[slot >> 1][2 * (slot & 1)], p); rf_load_a_inplace<1024>(WA[slot >> 1][2 * (slot & 1) + 1], p);
  };
  rf_for<0, DB_UPFRONT>(wload);
  // the zero frame of relu(h): everything, the interior is overwritten by stage 1's epilogue
  for (int i = tid; i < DB_HBYTES / 16; i += 256) ((uint4*)himg)[i] = make_uint4(0u, 0u, 0u, 0u);
  stamp(1);
  rf_wait<4 * DB_UPFRONT>();     // only the filter loads outstanding: every (older) patch deposit of this wavefront has landed
  rf_barrier();
  if (tid < 96) *(float4*)(bias_s + tid * 4) = bias_v;
  // ---- xp: the 2x2 mean of the RAW patch, fp32 from the stored 16-bit values, rounded once; thread = 8 channels of a pooled pixel ----
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int item = tid + 256 * k, p = item >> 4, sp = item & 15;
    const int pi = p >> 3, pj = p & 7;
    const int pp00 = (2 * pi + 1 + hf) * DB_PW + 2 * pj + 1;       // patch pixel of image pixel (8 hf + 2 pi, 2 pj)
    uint4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                  // x00, x10 (next row), x01 (next column), x11
      const int pp = pp00 + (q & 1) * DB_PW + (q >> 1);
      v[q] = *(const uint4*)(smem + pp * 256 + ((sp ^ (pp & 15)) << 4));
    }
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t w0 = (&v[0].x)[e], w1 = (&v[1].x)[e], w2 = (&v[2].x)[e], w3 = (&v[3].x)[e];
      o[e] = pack_h16x2((((h16_lo(w0) + h16_lo(w1)) + h16_lo(w2)) + h16_lo(w3)) * 0.25f,
                        (((h16_hi(w0) + h16_hi(w1)) + h16_hi(w2)) + h16_hi(w3)) * 0.25f);
    }
    const uint4 pk = make_uint4(o[0], o[1], o[2], o[3]);
    *(uint4*)(xps + p * 256 + ((sp ^ (p & 15)) << 4)) = pk;
    *(uint4*)(a.xp + (((long)n * 8 + 4 * hf + pi) * 8 + pj) * 128 + sp * 8) = pk;
  }
  rf_barrier();
  // the input ReLU once, in place (the DMA cannot apply it; on the fragments it would sit in the K loop)
  for (int i = tid; i < DB_XNPP * 16; i += 256) {
    uint4 v = *(uint4*)(smem + i * 16);
    v.x = relu_bf16x2(v.x); v.y = relu_bf16x2(v.y); v.z = relu_bf16x2(v.z); v.w = relu_bf16x2(v.w);
    *(uint4*)(smem + i * 16) = v;
  }
  rf_barrier();
  stamp(2);

  // ---- stage 1: NPT pixel tiles (one image row each) per group; see conv_rf.hip for the schedule of the K loop --------------------------
  // FIRST: the K loop issues the late filter loads (its own copy of the code: a load under an `if` would make the compiler merge "loaded"
  // and "kept" values of registers it believes are ready the moment the asm statement ends).  LAST: the K loop issues stage 2's first lap.
  auto group = [&](const int t0, auto npt_c, auto first_c, auto last_c, const int gi) __attribute__((always_inline)) {
    constexpr int NPT = decltype(npt_c)::value;
    constexpr bool FIRST = decltype(first_c)::value, LAST = decltype(last_c)::value;
    const unsigned lds_base = lds0;
    int ppl[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      const int t = t0 + pt, cr = t < 8 ? t + hf : (hf ? 0 : 8);       // tiles 0..7: the owned rows, tile 8: the halo row
      ppl[pt] = cr * DB_PW + r;
      asm volatile("" : "+v"(ppl[pt]));          // (opaque: the fragment addresses of a group must not be hoisted and spilled)
    }
    f32x4_t acc[NPT][4];                         // [pixel tile][channel tile]; written (not accumulated) by the first K-step
    auto xaddr = [&](int s, int pt, unsigned& out) __attribute__((always_inline)) {
      const int gk = kq * 18 + s, tap = gk >> 2, cq = gk & 3;
      const int t3 = (tap * 11) >> 5;            // tap / 3 for tap < 9
      const int stap = t3 * DB_PW + (tap - 3 * t3);
      const int slotk = cq * 4 + kc;
      unsigned tmp;
      // pp = ppl + tap offset;  out = lds0 + pp * 256 + ((slotk ^ (pp & 15)) << 4)
      asm volatile("v_add_u32 %0, %2, %3\n\tv_and_b32 %1, 15, %0\n\tv_xor_b32 %1, %1, %4\n\tv_lshl_add_u32 %1, %1, 4, %5\n\tv_lshl_add_u32 %0, %0, 8, %1"
                   : "=&v"(out), "=&v"(tmp) : "s"(stap), "v"(ppl[pt]), "v"(slotk), "s"(lds_base) : "memory");
    };
    unsigned ad[NPT];
    bf16x8_t xf[2][NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) xaddr(0, pt, ad[pt]);
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) rf_lds_read(xf[0][pt], ad[pt]);
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) xaddr(1, pt, ad[pt]);
    rf_for<0, 18>([&](auto ic) __attribute__((always_inline)) {
      constexpr int s = decltype(ic)::value;
      if constexpr (s + 1 < 18) {
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) rf_lds_read(xf[(s + 1) & 1][pt], ad[pt]);
      }
      if constexpr (FIRST) {
        if constexpr (s + DB_UPFRONT < 18) wload(std::integral_constant<int, s + DB_UPFRONT>{});
        rf_wait<4 * ((s + DB_UPFRONT < 18 ? s + DB_UPFRONT : 17) - s)>();
      }
      if constexpr (s + 1 < 18) asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(NPT) : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
          if constexpr (s == 0) rf_mfma_a0(acc[pt][ct], WA[s][ct], xf[s & 1][pt]);
          else if constexpr (s < DB_ASTEPS) rf_mfma_a(acc[pt][ct], WA[s][ct], xf[s & 1][pt]);
          else rf_mfma_v(acc[pt][ct], WV[s - DB_ASTEPS][ct], xf[s & 1][pt]);
        }
        if constexpr (s + 2 < 18) { if (ct < NPT) xaddr(s + 2, ct, ad[ct]); }
      }
      // K-step s < 16 has read WA[s] for the last time: ring slots 2s, 2s + 1 = stage 2's K-steps 2s, 2s + 1
      if constexpr (LAST && s < DB_ASTEPS) { w2load(std::integral_constant<int, 2 * s>{}); w2load(std::integral_constant<int, 2 * s + 1>{}); }
    });
    stamp(3 + 2 * gi);
    // ---- the two partial tiles meet in LDS: wavefront kq finishes half of the pair's tiles and sends the other half to its partner ----
    // (MFMA results read by non-MFMA instructions: the asm MFMAs are invisible to the compiler's hazard recogniser)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    // finished tile j of this wavefront: NPT = 4: pixel tile 2 kq + j, channel tile ct;  NPT = 1: pixel tile 0, channel tile 2 kq + j
    constexpr int NF = NPT == 4 ? 2 : 1, NC = NPT == 4 ? 4 : 2;
    f32x4_t mine[NF][NC];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        f32x4_t keep, send;
        if constexpr (NPT == 4) { keep = kq ? acc[2 + j][c] : acc[j][c]; send = kq ? acc[j][c] : acc[2 + j][c]; }
        else { keep = kq ? acc[0][2 + c] : acc[0][c]; send = kq ? acc[0][c] : acc[0][2 + c]; }
        mine[j][c] = keep;
        red[(wave * 8 + j * NC + c) * 64 + lane] = make_float4(send[0], send[1], send[2], send[3]);
      }
    rf_barrier();
    f32x4_t fin[NF][NC];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float4 o = red[((wave ^ 1) * 8 + j * NC + c) * 64 + lane];
        const f32x4_t ov = (f32x4_t){o.x, o.y, o.z, o.w};
        fin[j][c] = kq ? ov + mine[j][c] : mine[j][c] + ov;      // slice 0 + slice 1, as conv_rf_kernel sums them
      }
    rf_barrier();                                // the exchange buffer is free for the next group
    // ---- epilogue: + bias, one rounding; the owned rows to HBM, relu(h) of every row to the padded image of stage 2 ----
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int t = NPT == 4 ? t0 + 2 * kq + j : t0, ct = NPT == 4 ? c : 2 * kq + c;
        const int cr = t < 8 ? t + hf : (hf ? 0 : 8);
        const int c0 = cb * 64 + ct * 16 + 4 * kc;
        const float4 b4 = *(const float4*)(bias_s + c0);
        uint2 pk;
        pk.x = pack_h16x2(fin[j][c][0] + b4.x, fin[j][c][1] + b4.y);
        pk.y = pack_h16x2(fin[j][c][2] + b4.z, fin[j][c][3] + b4.w);
        if (t < 8) *(uint2*)(a.h + (((long)n * 16 + 7 * hf + cr) * 16 + r) * 128 + c0) = pk;
        pk.x = relu_bf16x2(pk.x); pk.y = relu_bf16x2(pk.y);
        const int pp = (cr + 1 - hf) * DB_PW + r + 1;
        *(uint2*)(himg + pp * 256 + (((c0 >> 3) ^ (pp & 15)) << 4) + (kc & 1) * 8) = pk;
      }
    stamp(4 + 2 * gi);
  };
  group(0, std::integral_constant<int, 4>{}, std::true_type{}, std::false_type{}, 0);
  group(4, std::integral_constant<int, 4>{}, std::false_type{}, std::false_type{}, 1);
  group(8, std::integral_constant<int, 1>{}, std::false_type{}, std::true_type{}, 2);
  rf_barrier();                                  // relu(h) is complete

  // ---- stage 2: this wavefront's 32 channels x the 32 pooled pixels; pixel tile pt = pooled rows 2 pt, 2 pt + 1 --------------------------
  int pq[2];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    pq[pt] = pt * 16 + r;
    asm volatile("" : "+v"(pq[pt]));             // (opaque: the 136 fragment addresses must not be hoisted and spilled)
  }
  auto xread = [&](auto ic, bf16x8_t (&xf)[2]) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value;
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      if constexpr (u < 4) {                     // shortcut: xp, channels u * 32 ..
        const int p = pq[pt];
        xf[pt] = *(const bf16x8_t*)(xps + p * 256 + (((u * 4 + kc) ^ (p & 15)) << 4));
      } else {                                   // Conv2: tap (uu, vv) of the 4x4 stride-2 window, channel quarter cq
        constexpr int s = u - 4, tap = s >> 2, cq = s & 3, uu = tap >> 2, vv = tap & 3;
        const int p = pq[pt];
        const int pp = (2 * (p >> 3) + uu) * DB_PW + 2 * (p & 7) + vv;
        xf[pt] = *(const bf16x8_t*)(himg + pp * 256 + (((cq * 4 + kc) ^ (pp & 15)) << 4));
      }
    }
  };
  // Conv2's reduction in the order of the tile kernel it replaces (conv_mfma_glds_kernel<64, 64, 2, 2, 2>: 64-deep K-tiles dealt
  // alternately to two groups of wavefronts, each summing its tiles in order from zero, group 0 + group 1 at the end): the K-tiles of
  // even and of odd index have their own accumulators here, so the block output keeps the four launches' BITS, not just their rounding points
  f32x4_t accs[2][2], acc2[2][2][2];             // [pixel tile][channel tile]: shortcut;  [K-tile parity][pixel tile][channel tile]: Conv2
  bf16x8_t xf2[2][2];
  xread(std::integral_constant<int, 0>{}, xf2[0]);
  rf_for<0, DB_STEPS2>([&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = u % DB_RING;
    if constexpr (u + 1 < DB_STEPS2) xread(std::integral_constant<int, u + 1>{}, xf2[(u + 1) & 1]);
    // loads retire in order: K-step u has landed once at most the loads of the K-steps behind it (u + 1 .. u + DB_RING - 1) are outstanding
    rf_wait<2 * ((u + DB_RING - 1 < DB_STEPS2 - 1 ? u + DB_RING - 1 : DB_STEPS2 - 1) - u)>();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        const i32x4_t& w = WA[slot >> 1][2 * (slot & 1) + ct];
        if constexpr (u == 0) rf_mfma_a0(accs[pt][ct], w, xf2[u & 1][pt]);
        else if constexpr (u < 4) rf_mfma_a(accs[pt][ct], w, xf2[u & 1][pt]);
        else if constexpr (u == 4 || u == 6) rf_mfma_a0(acc2[((u - 4) >> 1) & 1][pt][ct], w, xf2[u & 1][pt]);
        else rf_mfma_a(acc2[((u - 4) >> 1) & 1][pt][ct], w, xf2[u & 1][pt]);
      }
    if constexpr (u + DB_RING < DB_STEPS2) w2load(std::integral_constant<int, u + DB_RING>{});
  });
  stamp(9);
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  // ---- epilogue: t = bf16(shortcut + bs);  y = bf16(((even K-tiles + odd K-tiles) + b2) + t) ----
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int c0 = wave * 32 + ct * 16 + 4 * kc;
      const float4 b2 = *(const float4*)(bias_s + 128 + c0), bs = *(const float4*)(bias_s + 256 + c0);
      uint2 t;
      t.x = pack_h16x2(accs[pt][ct][0] + bs.x, accs[pt][ct][1] + bs.y);
      t.y = pack_h16x2(accs[pt][ct][2] + bs.z, accs[pt][ct][3] + bs.w);
      const f32x4_t c2 = acc2[0][pt][ct] + acc2[1][pt][ct];
      uint2 pk;
      pk.x = pack_h16x2((c2[0] + b2.x) + h16_lo(t.x), (c2[1] + b2.y) + h16_hi(t.x));
      pk.y = pack_h16x2((c2[2] + b2.z) + h16_lo(t.y), (c2[3] + b2.w) + h16_hi(t.y));
      const int p = pt * 16 + r;
      *(uint2*)(a.y + (((long)n * 8 + 4 * hf + (p >> 3)) * 8 + (p & 7)) * 128 + c0) = pk;
    }
  stamp(10);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

bool dblock2_takes(const rcgan_conv_desc* d) {
  if (!d || d->dtype != RCGAN_H16 || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->flags != RCGAN_CONV_IN_RELU) return false;
  if (!(d->n >= 1 && d->h == 16 && d->w == 16 && d->cin == 128 && d->cout == 128)) return false;
  return (long)d->n * d->h * d->w * d->cin < (1L << 31);
}

}  // namespace

extern "C" {

// d: D.Block.2.Conv1's descriptor (n x 16 x 16 x 128 -> 128, 3x3, RCGAN_CONV_IN_RELU, the build's 16-bit dtype); conv1_frag: its copy of
// rcgan_conv_rf_prepare / rcgan_fragments_prepare; dblock2_frag: what rcgan_fragments_prepare_dblock2 wrote for the current weights.
int rcgan_dblock2_ok(const rcgan_conv_desc* d, const void* conv1_frag, const void* dblock2_frag) {
  return dblock2_takes(d) && conv1_frag && dblock2_frag ? 1 : 0;
}

size_t rcgan_dblock2_fragment_bytes(void) { return (size_t)DB2_FRAG_ELEMS * sizeof(bf16_t); }      // the forward's copies, then the data gradient's

// h [n][16][16][128], xp [n][8][8][128] and y [n][8][8][128] are written: everything the block's (unfused) backward pass reads.
int rcgan_dblock2_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* conv1_frag, const void* dblock2_frag,
                      const float* bias1, const float* bias2, const float* bias_shortcut, void* h, void* xp, void* y) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, rcgan_dblock2_ok(d, conv1_frag, dblock2_frag), "not the 16x16x128 down block / missing fragment copies (rcgan_dblock2_ok)");
  RC_REQUIRE(ctx, x && bias1 && bias2 && bias_shortcut && h && xp && y, "null argument");
  Db2Args a;
  a.x = (const bf16_t*)x; a.w1 = (const bf16_t*)conv1_frag; a.w2 = (const bf16_t*)dblock2_frag;
  a.b1 = bias1; a.b2 = bias2; a.bs = bias_shortcut;
  a.h = (bf16_t*)h; a.xp = (bf16_t*)xp; a.y = (bf16_t*)y;
  a.zero = (const bf16_t*)ctx->zero_page;
  a.stamps = (unsigned long long*)ctx->dbg_stamps;
  static bool attr_set = false;
  if (!attr_set) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_dblock2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DB_LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL(conv_dblock2_kernel, dim3(2 * d->n), dim3(256), DB_LDS, ctx->stream, a);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
