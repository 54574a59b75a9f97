// D.Block.2 of the CIFAR discriminator, the 16x16x128 -> 8x8x128 down block (conv_dblock2.hip has the forward), DATA GRADIENT, as ONE launch:
//     dh  = 16bit([h > 0] . (Conv2 + pool)^T(dy))                   sub-pixel form: pixel (2i + ph, 2j + pw) gathers 2x2 pooled pixels of dy with
//                                                                   the summed, transposed filters of its phase (K = 512); Conv1's filter gradient reads it
//     dxp = 16bit(Shortcut^T(dy))                                   1x1 at 8 x 8; a rounding point only: it stays in LDS
//     dx  = 16bit(16bit([x > 0] . Conv1^T(dh)) + 0.25 spread2x2(dxp))
// As four launches (the 64 x 64 tile kernel in its phase form, conv_rf_kernel's data gradient, the tile kernel on the 1x1, the pool's adjoint
// accumulated into dx) every launch pays dispatch, a cold patch and filter fetch, fill and drain.  The geometry is the forward's in mirror image:
//   * workgroup (image, half) owns 8 rows of dx and of dh and computes 9 rows of dh (rows 0..8 / 7..15: one halo row, 12.5 % more sub-pixel
//     work) from pooled dy rows 0..4 / 3..7; nothing is exchanged between workgroups, exactly one workgroup writes each element;
//   * stage 1: a wavefront owns 32 channels.  4 K-steps of the shortcut over the 32 pooled pixels of the owned rows, then the four (row parity,
//     column parity) classes of the 9 rows, 16 K-steps each, 3 or 2 pixel tiles of (2 rows x 8 columns of one parity).  The filters (32 KB
//     + 512 KB per workgroup) stream through a ring of 32 K-steps in the 256 AccVGPRs, as the forward's stage 2.  h (the mask) arrives by
//     LDS-DMA in the buffer stage 2 exchanges partial tiles through.  The epilogue of a class rounds, masks, stores the owned rows and leaves
//     all nine in LDS as the zero-padded 10 x 18 patch of stage 2;
//   * stage 2 is conv_rf_kernel<128, 16>'s K loop, exchange and sum (conv_rf.hip) on that patch with Conv1's rotated fragments, which the last
//     lap of the ring loads into the registers it frees.  Its epilogue masks by x, rounds, adds 0.25 dxp as resample2_vec_kernel does, rounds.
// Rounding points and fp32 summation orders are the four launches' at the shapes of the training step (the phase form and the 1x1 on
// conv_mfma_glds_kernel<64, 64, 2, 1, *>: one chain over the K-tiles in order from zero; Conv1: slice 0 + slice 1), so dh and dx have their bits.
#include <type_traits>

#include "conv_mfma.h"
#include "mfma_util.h"
#include "rf_asm.h"

namespace {

constexpr int BW_PW = 18;                                  // stage 2's padded row: 16 pixels + two halo columns
constexpr int BW_HNPP = 10 * BW_PW;                        // the dh patch: image rows 8 hf - 1 .. 8 hf + 8
constexpr int BW_HBYTES = BW_HNPP * 256;
constexpr int BW_YW = 10;                                  // the dy patch: pooled rows -1 .. 4 / 3 .. 8, pooled columns -1 .. 8
constexpr int BW_YNPP = 6 * BW_YW;
constexpr int BW_YBYTES = 16 * 1024;
constexpr int BW_XPBYTES = 32 * 256;                       // dxp of the 4 x 8 pooled pixels under the owned rows
constexpr int BW_RED = 4 * 16 * 64 * 16;                   // stage 2's partial-tile exchange (conv_rf.hip: RF_RED); stage 1: the 9 x 16 pixels of h
constexpr int BW_MASK = 9 * 16 * 256;
constexpr int BW_LDS = BW_HBYTES + BW_YBYTES + BW_XPBYTES + BW_RED;
constexpr int BW_RING = 32;                                // stage 1: K-steps in flight
constexpr int BW_STEPS = 4 + 64;                           // stage 1: shortcut K-steps, then four classes of 16
constexpr int BW_LAST = BW_STEPS - BW_RING;                // first K-step behind which no ring load is issued: stage 2's filters instead
static_assert(BW_YNPP * 256 <= BW_YBYTES && BW_MASK <= BW_RED && BW_HBYTES % 1024 == 0, "LDS regions");
static_assert(BW_LDS <= 160 * 1024, "LDS of one CU");

struct Db2BwdArgs {
  const bf16_t *dy, *h, *x;      // [n][8][8][128], [n][16][16][128] x 2
  const bf16_t* w1;              // Conv1: the data gradient's fragments of rcgan_conv_rf_prepare
  const bf16_t* w2;              // the block's copies (rf_asm.h: dblock2_frag_items)
  bf16_t *dh, *dx;               // [n][16][16][128]
  const bf16_t* zero;            // >= 16 zero bytes (halo source)
  unsigned long long* stamps;    // diagnostics (rcgan_debug_stamps): 16 s_memtime stamps per workgroup, normally null
};

// loads issued behind K-step u's ring loads when K-step u waits for them: the ring loads of the K-steps behind it, and stage 2's filters (four
// loads behind every second K-step of the last lap)
constexpr int bw_behind(int u) {
  return 2 * ((u + BW_RING - 1 < BW_STEPS - 1 ? u + BW_RING - 1 : BW_STEPS - 1) - u) + (u > BW_LAST ? 4 * ((u - BW_LAST) / 2) : 0);
}

__global__ __launch_bounds__(256) void conv_dblock2_bwd_kernel(Db2BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // [dy patch][h, then the exchange][dh patch][dxp]: the LDS-DMA targets first
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = wave & 1, cb = wave >> 1;                 // stage 2: K slice, 64-channel block
  const int r = lane & 15, kc = lane >> 4;
  const int n = (int)blockIdx.x >> 1, hf = (int)blockIdx.x & 1;      // computed row cr of dh is image row 7 hf + cr, patch row cr + 1 - hf
  unsigned char* const dyp = smem;
  unsigned char* const hmask = dyp + BW_YBYTES;
  unsigned char* const dhp = hmask + BW_RED;
  unsigned char* const dxps = dhp + BW_HBYTES;
  float4* const red = (float4*)hmask;
  auto stamp = [&](int k) __attribute__((always_inline)) {
    if (a.stamps && tid == 0) a.stamps[(long)blockIdx.x * 16 + k] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);

  i32x4_t WA[16][4], WV[2][4];
  const bf16_t* const w1l = a.w1 + ((long)(cb * 2 + kq) * 18) * (4 * 512) + lane * 8;
  const bf16_t* const wsl = a.w2 + DB2_FRAG_SHORT_BWD + (long)wave * (4 * 1024) + lane * 8;           // K-step u < 4: + u * 1024
  // class q = 2 e + pw (e: parity of cr, pw: of the column) is phase (ph, pw) of the summed filters, ph = parity of 7 hf + cr
  const bf16_t* const w2l = a.w2 + DB2_FRAG_CONV2_BWD + (long)wave * (16 * 1024) + lane * 8;
  const long cls_e0 = (long)(2 * hf) * (64 * 1024), cls_e1 = (long)(2 * (1 - hf)) * (64 * 1024);

  // ---- dy and h by LDS-DMA (conv_rf.hip): 16-byte slots XOR-swizzled with the pixel index on the source side ----
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  {
    const bf16_t* const img = a.dy + (long)n * 64 * 128;
    const int pr0 = hf ? 3 : -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = i * 4 + wave;
      if (q < BW_YNPP * 16 / 64) {                 // (wavefront-uniform)
        const int c = q * 64 + lane, pp = c >> 4, sp = c & 15;
        const int pr = pp / BW_YW, pc = pp - pr * BW_YW;
        const int ih = pr0 + pr, iw = pc - 1;
        const bool ok = ih >= 0 && ih < 8 && iw >= 0 && iw < 8;
        const int off = ((ih * 8 + iw) * 128 + ((sp ^ (pp & 15)) << 3)) * 2;
        const char* src = ok ? (const char*)img + off : (const char*)a.zero;
        glds16_asm(src, lds0 + q * 1024);
      }
    }
    const bf16_t* const himg = a.h + ((long)n * 16 + 7 * hf) * 16 * 128;
#pragma unroll
    for (int i = 0; i < BW_MASK / 4096; ++i) {
      const int q = i * 4 + wave;
      const int c = q * 64 + lane, hp = c >> 4, sp = c & 15;           // hp = cr * 16 + column
      glds16_asm((const char*)himg + (hp * 128 + ((sp ^ (hp & 15)) << 3)) * 2, lds0 + BW_YBYTES + q * 1024);
    }
  }
  // K-step u of stage 1 lives in ring slot (u + 28) % 32 = WA[slot / 2][2 * (slot & 1) + channel tile]: the last four K-steps use the last
  // four slots, so the last lap frees WA[0], WA[1], ... in the order stage 2 reads them
  auto w1src = [&](auto ic) __attribute__((always_inline)) -> const bf16_t* {
    constexpr int u = decltype(ic)::value;
    if constexpr (u < 4) return wsl + u * 1024;
    else return w2l + ((u - 4) >> 5 ? cls_e1 : cls_e0) + (((u - 4) >> 4) & 1) * (64 * 1024) + ((u - 4) & 15) * 1024;
  };
  auto ring_first = [&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = (u + 28) % BW_RING;
    const bf16_t* const p = w1src(ic);
    rf_load_a<0>(WA[slot >> 1][2 * (slot & 1)], p); rf_load_a<1024>(WA[slot >> 1][2 * (slot & 1) + 1], p);
  };
  auto ring_load = [&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = (u + 28) % BW_RING;
    const bf16_t* const p = w1src(ic);
    rf_load_a_inplace<0>(WA[slot >> 1][2 * (slot & 1)], p); rf_load_a_inplace<1024>(WA[slot >> 1][2 * (slot & 1) + 1], p);
  };
  // stage 2's K-step s (conv_rf.hip: 18 per slice, 16 in AccVGPRs) into the registers the ring has finished with
  auto w2load = [&](auto ic) __attribute__((always_inline)) {
    constexpr int s = decltype(ic)::value;
    const bf16_t* const p = w1l + s * (4 * 512);
    if constexpr (s < 16) {
      rf_load_a_inplace<0>(WA[s][0], p); rf_load_a_inplace<1024>(WA[s][1], p);
      rf_load_a_inplace<2048>(WA[s][2], p); rf_load_a_inplace<3072>(WA[s][3], p);
    } else {
      rf_load_v<0>(WV[s - 16][0], p); rf_load_v<1024>(WV[s - 16][1], p); rf_load_v<2048>(WV[s - 16][2], p); rf_load_v<3072>(WV[s - 16][3], p);
    }
  };
  rf_for<0, BW_RING>(ring_first);
  // the zero frame of the dh patch: everything, the interior is overwritten by stage 1's epilogues
  for (int i = tid; i < BW_HBYTES / 16; i += 256) ((uint4*)dhp)[i] = make_uint4(0u, 0u, 0u, 0u);
  stamp(1);
  // at most 4 + 9 deposits in front of the 64 filter loads: with 48 outstanding every deposit of this wavefront has landed
  rf_wait<48>();
  rf_barrier();
  stamp(2);

  // ---- stage 1 ----
  int pqs[2], ppq[2][3];                         // patch pixel of tap (0, 0): shortcut tile pt; class parity e, pixel tile pt (pw = 0)
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const int p = pt * 16 + r;
    pqs[pt] = ((p >> 3) + 1) * BW_YW + (p & 7) + 1;
    asm volatile("" : "+v"(pqs[pt]));            // (opaque: the fragment addresses must not be hoisted and spilled)
  }
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int pt = 0; pt < 3; ++pt) {
      int cr = 2 * (2 * pt + (r >> 3)) + e;      // lanes 0..7: one row, lanes 8..15: the next of the same parity
      cr = cr > 8 ? 8 : cr;                      // (the fifth row pair of the even class has one row: its other half computes a copy nobody stores)
      ppq[e][pt] = ((cr + 1 - hf) >> 1) * BW_YW + (r & 7);
      asm volatile("" : "+v"(ppq[e][pt]));
    }
  auto xread = [&](auto ic, bf16x8_t (&xf)[3]) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value;
    if constexpr (u < 4) {                       // shortcut: channels u * 32 ..
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        const int pp = pqs[pt];
        xf[pt] = *(const bf16x8_t*)(dyp + pp * 256 + (((u * 4 + kc) ^ (pp & 15)) << 4));
      }
    } else {                                     // class q, tap (ta, tb) of the 2x2 window, channel quarter cq
      constexpr int s = u - 4, q = s >> 4, ks = s & 15, ta = ks >> 3, tb = (ks >> 2) & 1, cq = ks & 3, e = q >> 1, pw = q & 1;
#pragma unroll
      for (int pt = 0; pt < (e ? 2 : 3); ++pt) {
        const int pp = ppq[e][pt] + ta * BW_YW + tb + pw;
        xf[pt] = *(const bf16x8_t*)(dyp + pp * 256 + (((cq * 4 + kc) ^ (pp & 15)) << 4));
      }
    }
  };
  f32x4_t accs[2][2], acc1[3][2];                // [pixel tile][channel tile]: shortcut; the current class
  bf16x8_t xf1[2][3];
  // rows (16-lane groups) of a channel-tile pair after swap16 (mfma_util.h): 8 consecutive channels of the wavefront's 32
  const int c8 = wave * 32 + (kc & 1) * 16 + (kc >> 1) * 8;
  xread(std::integral_constant<int, 0>{}, xf1[0]);
  rf_for<0, BW_STEPS>([&](auto ic) __attribute__((always_inline)) {
    constexpr int u = decltype(ic)::value, slot = (u + 28) % BW_RING;
    constexpr int q = u < 4 ? 0 : (u - 4) >> 4, ks = u < 4 ? u : (u - 4) & 15, e = q >> 1, pw = q & 1;
    constexpr int NT = u < 4 ? 2 : (e ? 2 : 3);
    if constexpr (u + 1 < BW_STEPS) xread(std::integral_constant<int, u + 1>{}, xf1[(u + 1) & 1]);
    // loads retire in order: K-step u has landed once at most the loads issued behind it are outstanding
    rf_wait<bw_behind(u)>();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int pt = 0; pt < NT; ++pt) {
        const i32x4_t& w = WA[slot >> 1][2 * (slot & 1) + ct];
        if constexpr (u == 0) rf_mfma_a0(accs[pt][ct], w, xf1[u & 1][pt]);
        else if constexpr (u < 4) rf_mfma_a(accs[pt][ct], w, xf1[u & 1][pt]);
        else if constexpr (ks == 0) rf_mfma_a0(acc1[pt][ct], w, xf1[u & 1][pt]);
        else rf_mfma_a(acc1[pt][ct], w, xf1[u & 1][pt]);
      }
    if constexpr (u + BW_RING < BW_STEPS) ring_load(std::integral_constant<int, u + BW_RING>{});
    else if constexpr ((u - BW_LAST) & 1) w2load(std::integral_constant<int, (u - BW_LAST) / 2>{});
    if constexpr (u == BW_STEPS - 1) { w2load(std::integral_constant<int, 16>{}); w2load(std::integral_constant<int, 17>{}); }
    if constexpr (u == 3) {
      // ---- dxp = 16bit(shortcut), kept in LDS ----
      // (MFMA results read by non-MFMA instructions: the asm MFMAs are invisible to the compiler's hazard recogniser)
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int p = pt * 16 + r, c0 = wave * 32 + ct * 16 + 4 * kc;
          uint2 pk;
          pk.x = pack_h16x2(accs[pt][ct][0] + 0.f, accs[pt][ct][1] + 0.f);
          pk.y = pack_h16x2(accs[pt][ct][2] + 0.f, accs[pt][ct][3] + 0.f);
          *(uint2*)(dxps + p * 256 + (((c0 >> 3) ^ (p & 15)) << 4) + (kc & 1) * 8) = pk;
        }
      stamp(3);
    }
    if constexpr (u >= 4 && ks == 15) {
      // ---- dh of class q: one rounding, the mask, the owned rows to HBM, every row to stage 2's patch ----
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int pt = 0; pt < NT; ++pt) {
        float x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          x[k] = acc1[pt][0][k] + 0.f;
          y[k] = acc1[pt][1][k] + 0.f;
          swap16(x[k], y[k]);
        }
        const int cr = 2 * (2 * pt + (r >> 3)) + e, col = 2 * (r & 7) + pw;
        if (cr <= 8) {
          const int hp = cr * 16 + col;
          const uint4 m = *(const uint4*)(hmask + hp * 256 + (((c8 >> 3) ^ (hp & 15)) << 4));
          const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            if (!(h16_lo(mw[k]) > 0.f)) x[2 * k] = 0.f;
            if (!(h16_hi(mw[k]) > 0.f)) x[2 * k + 1] = 0.f;
            if (!(h16_lo(mw[2 + k]) > 0.f)) y[2 * k] = 0.f;
            if (!(h16_hi(mw[2 + k]) > 0.f)) y[2 * k + 1] = 0.f;
          }
          const uint4 pk = make_uint4(pack_h16x2(x[0], x[1]), pack_h16x2(x[2], x[3]), pack_h16x2(y[0], y[1]), pack_h16x2(y[2], y[3]));
          if (hf ? cr >= 1 : cr <= 7) *(uint4*)(a.dh + (((long)n * 16 + 7 * hf + cr) * 16 + col) * 128 + c8) = pk;
          const int pp = (cr + 1 - hf) * BW_PW + col + 1;
          *(uint4*)(dhp + pp * 256 + (((c8 >> 3) ^ (pp & 15)) << 4)) = pk;
        }
      }
      stamp(4 + q);
    }
  });
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // stage 2's filters are in their registers
  rf_barrier();                                           // the dh patch is complete, h is dead: its buffer is the exchange's
  stamp(8);

  // ---- stage 2: conv_rf_kernel<128, 16>'s group (conv_rf.hip has the schedule of the K loop), two groups of 64 pixels ----
  auto group = [&](const int g) __attribute__((always_inline)) {
    const unsigned lds_base = lds0 + BW_YBYTES + BW_RED;       // the dh patch
    int ppl[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int p = g * 64 + pt * 16 + r;
      ppl[pt] = (p >> 4) * BW_PW + (p & 15);
      asm volatile("" : "+v"(ppl[pt]));          // (opaque: the 72 fragment addresses of a group must not be hoisted and spilled)
    }
    f32x4_t acc[4][4];                           // [pixel tile][channel tile]; written (not accumulated) by the first K-step
    auto xaddr = [&](int s, int pt, unsigned& out) __attribute__((always_inline)) {
      const int gk = kq * 18 + s, tap = gk >> 2, cq = gk & 3;
      const int t3 = (tap * 11) >> 5;            // tap / 3 for tap < 9
      const int stap = t3 * BW_PW + (tap - 3 * t3);
      const int slotk = cq * 4 + kc;
      unsigned tmp;
      // pp = ppl + tap offset;  out = lds0 + pp * 256 + ((slotk ^ (pp & 15)) << 4)
      asm volatile("v_add_u32 %0, %2, %3\n\tv_and_b32 %1, 15, %0\n\tv_xor_b32 %1, %1, %4\n\tv_lshl_add_u32 %1, %1, 4, %5\n\tv_lshl_add_u32 %0, %0, 8, %1"
                   : "=&v"(out), "=&v"(tmp) : "s"(stap), "v"(ppl[pt]), "v"(slotk), "s"(lds_base) : "memory");
    };
    unsigned ad[4];
    bf16x8_t xf[2][4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) xaddr(0, pt, ad[pt]);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) rf_lds_read(xf[0][pt], ad[pt]);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) xaddr(1, pt, ad[pt]);
    rf_for<0, 18>([&](auto ic) __attribute__((always_inline)) {
      constexpr int s = decltype(ic)::value;
      if constexpr (s + 1 < 18) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) rf_lds_read(xf[(s + 1) & 1][pt], ad[pt]);
      }
      if constexpr (s + 1 < 18) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
          if constexpr (s == 0) rf_mfma_a0(acc[pt][ct], WA[s][ct], xf[s & 1][pt]);
          else if constexpr (s < 16) rf_mfma_a(acc[pt][ct], WA[s][ct], xf[s & 1][pt]);
          else rf_mfma_v(acc[pt][ct], WV[s - 16][ct], xf[s & 1][pt]);
        }
        if constexpr (s + 2 < 18) xaddr(s + 2, ct, ad[ct]);
      }
    });
    stamp(9 + 2 * g);
    // ---- the two partial tiles meet in LDS: slice order, every wavefront finishes two pixel tiles x four channel tiles ----
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        red[(wave * 16 + pt * 4 + ct) * 64 + lane] = make_float4(acc[pt][ct][0], acc[pt][ct][1], acc[pt][ct][2], acc[pt][ct][3]);
    rf_barrier();
    f32x4_t fin[4][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int pt = kq * 2 + j;
        float4 sum = red[((cb * 2) * 16 + pt * 4 + ct) * 64 + lane];
        const float4 v = red[((cb * 2 + 1) * 16 + pt * 4 + ct) * 64 + lane];
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        fin[ct][j] = (f32x4_t){sum.x, sum.y, sum.z, sum.w};
      }
    rf_barrier();                                // the exchange buffer is free for the next group
    // ---- epilogue: dxc = 16bit([x > 0] . sum) as conv_epilogue forms it; dx = 16bit(0.25 dxp + dxc) as resample2_vec_kernel<T, 1> ----
    uint4 xm[2][2];
    long goff[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int px = g * 64 + kq * 32 + j * 16 + r;      // pixel of the owned 8 x 16
        goff[j][p] = (((long)n * 256 + hf * 128 + px) * 128) + cb * 64 + (2 * p + (kc & 1)) * 16 + (kc >> 1) * 8;
        xm[j][p] = *(const uint4*)(a.x + goff[j][p]);
      }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          x[k] = fin[2 * p][j][k] + 0.f;
          y[k] = fin[2 * p + 1][j][k] + 0.f;
          swap16(x[k], y[k]);
        }
        const uint32_t mw[4] = {xm[j][p].x, xm[j][p].y, xm[j][p].z, xm[j][p].w};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (!(h16_lo(mw[k]) > 0.f)) x[2 * k] = 0.f;
          if (!(h16_hi(mw[k]) > 0.f)) x[2 * k + 1] = 0.f;
          if (!(h16_lo(mw[2 + k]) > 0.f)) y[2 * k] = 0.f;
          if (!(h16_hi(mw[2 + k]) > 0.f)) y[2 * k + 1] = 0.f;
        }
        const uint32_t dc[4] = {pack_h16x2(x[0], x[1]), pack_h16x2(x[2], x[3]), pack_h16x2(y[0], y[1]), pack_h16x2(y[2], y[3])};
        const int px = g * 64 + kq * 32 + j * 16 + r;
        const int pl = (px >> 5) * 8 + ((px & 15) >> 1);   // pooled pixel under it
        const int ch8 = cb * 8 + (2 * p + (kc & 1)) * 2 + (kc >> 1);
        const uint4 dp = *(const uint4*)(dxps + pl * 256 + ((ch8 ^ (pl & 15)) << 4));
        const uint32_t dw[4] = {dp.x, dp.y, dp.z, dp.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float lo = h16_lo(dw[k]) * 0.25f, hi = h16_hi(dw[k]) * 0.25f;
          lo += h16_lo(dc[k]); hi += h16_hi(dc[k]);
          o[k] = pack_h16x2(lo, hi);
        }
        *(uint4*)(a.dx + goff[j][p]) = make_uint4(o[0], o[1], o[2], o[3]);
      }
    stamp(10 + 2 * g);
  };
  group(0);
  group(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

extern "C" {

// d, conv1_frag, dblock2_frag: as rcgan_dblock2_fwd.  dy [n][8][8][128]: the gradient of the block's output; h, x [n][16][16][128]: Conv1's
// output and the block's input of the forward pass (masks).  dh [n][16][16][128] and dx [n][16][16][128] are written (dx is not accumulated into).
int rcgan_dblock2_bwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* h, const void* x, const void* conv1_frag,
                      const void* dblock2_frag, void* dh, void* dx) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, rcgan_dblock2_ok(d, conv1_frag, dblock2_frag), "not the 16x16x128 down block / missing fragment copies (rcgan_dblock2_ok)");
  RC_REQUIRE(ctx, dy && h && x && dh && dx, "null argument");
  Db2BwdArgs a;
  a.dy = (const bf16_t*)dy; a.h = (const bf16_t*)h; a.x = (const bf16_t*)x;
  a.w1 = (const bf16_t*)conv1_frag + (size_t)9 * 128 * 128;
  a.w2 = (const bf16_t*)dblock2_frag;
  a.dh = (bf16_t*)dh; a.dx = (bf16_t*)dx;
  a.zero = (const bf16_t*)ctx->zero_page;
  a.stamps = (unsigned long long*)ctx->dbg_stamps;
  static bool attr_set = false;
  if (!attr_set) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_dblock2_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BW_LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL(conv_dblock2_bwd_kernel, dim3(2 * d->n), dim3(256), BW_LDS, ctx->stream, a);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
