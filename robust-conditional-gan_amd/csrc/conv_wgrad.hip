// Filter gradients on the matrix cores of gfx950 (CDNA4): kernels, slab reduction, routing, launchers and the two entry points
// rcgan_conv2d_bwd_weight / rcgan_conv2d_bwd_weight_group.  (The nine-tap kernel has its own file, conv_wgrad9.hip.)
//
// Filter-gradient kernel: dW[tap][ci][co] = sum_m X[pix(m,tap)][ci] * dY[m][co], a GEMM whose
//   reduction runs over pixels.  Both operands are channel-contiguous in HBM but the MFMA wants
//   them pixel(k)-contiguous per lane; tiles are staged as [pixel][channel] and the fragments are
//   read with ds_read_b64_tr_b16 (the gfx950 LDS transpose read).  Pixel ranges are split across
//   blocks into fp32 slabs that a second kernel reduces (deterministic, no atomics).
//
// Order of the file: the per-tap, three-tap and grouped kernels; the slab reductions; which kernel a posed problem gets and its plan
// (mfma_wgrad_choose, mfma_wgrad_plan) and the launchers; posing a layer (wgrad_pose); the one-layer entry point; the group call as
// plan (wgrad_group_plan: decides everything, launches nothing) and issue (wgrad_group_issue).
#include "conv_wgrad.h"
#include "mfma_util.h"
#include "conv_image.h"
#include "head_rider.h"

template <typename T> int colsum_launch(rcgan_ctx*, const T*, long, int, float*, int, float*);      // conv_direct.hip

#define WG_PITCH 144          // elements per LDS row in the wgrad kernel (128 + 16 pad = 288 B)

__device__ __forceinline__ bf16x8_t frag_tr(const bf16_t* base /* &tile[row0][ch0] */, int lane, int use_tr) {
  // returns, for lane (g = lane>>4, i = lane&15), channel ch0+i at k-slots {g*4+e} U {16+g*4+e}, e=0..3
  const int g = lane >> 4, i = lane & 15;
  s16x8_t r;
  if (use_tr) {
    const bf16_t* p = base + (g * 4 + (i >> 2)) * WG_PITCH + (i & 3) * 4;
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * WG_PITCH));
    r = (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = (e < 4) ? (g * 4 + e) : (16 + g * 4 + (e - 4));
      r[e] = (short)base[row * WG_PITCH + i];
    }
  }
  return __builtin_bit_cast(bf16x8_t, r);
}

// block tile: 128 ci x 128 co for one tap; 4 waves as 2 (ci) x 2 (co), wave tile 64 x 64
__global__ __launch_bounds__(256) void conv_mfma_wgrad_kernel(MfmaWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Xs = (bf16_t*)smem;                    // [2][64][WG_PITCH]
  bf16_t* Ys = Xs + 2 * 64 * WG_PITCH;           // [2][64][WG_PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave & 1, wo = wave >> 1;
  const int nci = a.Cin / 128, nco = a.Cout / 128;
  int b = blockIdx.x;
  const int cot = b % nco; b /= nco;
  const int cit = b % nci; b /= nci;
  const int tap = b;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int ci0 = cit * 128, co0 = cot * 128;
  const long mb = (long)blockIdx.y * a.m_chunk;
  long me = mb + a.m_chunk;
  if (me > a.M) me = a.M;
  const int Hs = a.up ? (a.H >> 1) : a.H, Ws = a.up ? (a.W >> 1) : a.W;
  const int chunk = tid & 15, lrow = tid >> 4;   // 16 chunks of 8 channels, 16 rows per pass, 4 passes

  uint4 rx[4], ry[4];
  auto load_tile = [&](long p0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long m = p0 + lrow + 16 * i;
      uint4 vx = make_uint4(0, 0, 0, 0), vy = make_uint4(0, 0, 0, 0);
      if (m < me) {
        int ow, oh, n;
        decode_pix(m, a.H, a.W, a.lh, a.lw, n, oh, ow);
        int ih = oh + kh - a.PT, iw = ow + kw - a.PL;
        if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
          if (a.up) { ih >>= 1; iw >>= 1; }
          vx = *(const uint4*)(a.x + (unsigned)((((unsigned)n * Hs + ih) * Ws + iw) * a.Cin + ci0 + chunk * 8));
          if (a.relu_in) { vx.x = relu_bf16x2(vx.x); vx.y = relu_bf16x2(vx.y); vx.z = relu_bf16x2(vx.z); vx.w = relu_bf16x2(vx.w); }
        }
        vy = *(const uint4*)(a.dy + (unsigned)((unsigned)m * a.Cout + co0 + chunk * 8));
      }
      rx[i] = vx; ry[i] = vy;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(uint4*)(Xs + ((long)buf * 64 + lrow + 16 * i) * WG_PITCH + chunk * 8) = rx[i];
      *(uint4*)(Ys + ((long)buf * 64 + lrow + 16 * i) * WG_PITCH + chunk * 8) = ry[i];
    }
  };

  f32x4_t acc[4][4];   // [co tile][ci tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const long ntile = (me - mb + 63) / 64;
  if (ntile > 0) {
    load_tile(mb);
    store_tile(0);
  }
  __syncthreads();
  for (long t = 0; t < ntile; ++t) {
    const int buf = (int)(t & 1);
    if (t + 1 < ntile) load_tile(mb + (t + 1) * 64);
    const bf16_t* Xb = Xs + (long)buf * 64 * WG_PITCH + wi * 64;
    const bf16_t* Yb = Ys + (long)buf * 64 * WG_PITCH + wo * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t yf[4], xf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) yf[i] = frag_tr(Yb + ks * 32 * WG_PITCH + i * 16, lane, a.use_tr);
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[j] = frag_tr(Xb + ks * 32 * WG_PITCH + j * 16, lane, a.use_tr);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma16(yf[i], xf[j], acc[i][j]);
    }
    if (t + 1 < ntile) store_tile(buf ^ 1);
    __syncthreads();
  }
  // D[row = co (4*(lane>>4)+r)][col = ci (lane&15)]
  float* slab = a.slab + (long)blockIdx.y * a.slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + wo * 64 + i * 16 + (lane >> 4) * 4;
      const int ci = ci0 + wi * 64 + j * 16 + (lane & 15);
      float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      *(float4*)(slab + ((long)tap * a.Cin + ci) * a.Cout + co) = v;
    }
}


// ---------------------------------------------------------------------------------------------
// filter gradient, direct-to-LDS variant.  Tiles are [64 pixels][128 channels] = 256-B rows, deposited
// 4 rows per wavefront instruction.  16-B slot s of row r is stored at slot s ^ ((r & 7) << 1): the eight
// rows a ds_read_b64_tr_b16 half-wave touches then fall into eight distinct 32-B bank segments.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8_t frag_tr_swz(const unsigned char* tile, int row0, int slot0, int lane, int use_tr, int relu) {
  // lane (g = lane>>4, i = lane&15): channel = 8*slot0 + i (slot0 even), k-slots {g*4+e} U {16+g*4+e}
  const int g = lane >> 4, i = lane & 15;
  s16x8_t r;
  if (use_tr) {
    const int row = row0 + g * 4 + (i >> 2);
    const int sw = (row & 7) << 1;
    const unsigned char* p = tile + row * 256 + (((slot0 + ((i & 3) >> 1)) ^ sw) << 4) + (i & 1) * 8;
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * 256));
    r = (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = row0 + ((e < 4) ? (g * 4 + e) : (16 + g * 4 + (e - 4)));
      const int slot = (slot0 + (i >> 3)) ^ ((row & 7) << 1);
      r[e] = *(const short*)(tile + row * 256 + (slot << 4) + (i & 7) * 2);
    }
  }
  if (relu) {
    uint4 v = __builtin_bit_cast(uint4, r);
    v.x = relu_bf16x2(v.x); v.y = relu_bf16x2(v.y); v.z = relu_bf16x2(v.z); v.w = relu_bf16x2(v.w);
    r = __builtin_bit_cast(s16x8_t, v);
  }
  return __builtin_bit_cast(bf16x8_t, r);
}

template <int NS>
__device__ __forceinline__ void wgrad_glds_body(const MfmaWgradArgs& a, const unsigned bx, const unsigned by) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TILE = 32 * 256;                 // bytes per operand per stage: 32 pixels x 128 channels
  constexpr int STAGE = 2 * TILE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave & 1, wo = wave >> 1;
  const int nci = a.Cin / 128, nco = a.Cout / 128;
  int b = (int)bx;
  const int cot = b % nco; b /= nco;
  const int cit = b % nci; b /= nci;
  const int tap = b;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int ci0 = cit * 128, co0 = cot * 128;
  const long mb = (long)by * a.m_chunk;
  long me = mb + a.m_chunk;
  if (me > a.M) me = a.M;
  const int Hs = a.up ? (a.H >> 1) : a.H, Ws = a.up ? (a.W >> 1) : a.W;
  const int lrow = lane >> 4, pos = lane & 15;
  const int dh = kh - a.PT, dw = kw - a.PL;

  // this lane deposits 16-B slot `pos` of rows r_i = (wave*2+i)*4 + lrow, i = 0,1, of both operand tiles
  int r_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave * 2 + i) * 4 + lrow;
    r_off[i] = (pos ^ ((row & 7) << 1)) * 8;     // source-side swizzle (channel offset)
  }
  // (the geometry pinned in scalar registers: see wgrad3_body)
  const bf16_t* xbase = a.x + ci0;
  const bf16_t* ybase = a.dy + co0;
  const bf16_t* azero = a.zero;
  int aH = a.H, aW = a.W, aCin = a.Cin, aCout = a.Cout, alw = a.lw, alh = a.lh, aup = a.up;
  asm volatile("" : "+s"(xbase), "+s"(ybase), "+s"(azero), "+s"(aH), "+s"(aW), "+s"(aCin), "+s"(aCout), "+s"(alw), "+s"(alh), "+s"(aup));
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  long i_p0 = mb;
  auto issue = [&](int buf) {
    const unsigned stage = lds0 + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long m = i_p0 + (wave * 2 + i) * 4 + lrow;
      const bf16_t* px = azero;
      const bf16_t* py = azero;
      if (m < me) {
        int ow, oh, n;
        decode_pix(m, aH, aW, alh, alw, n, oh, ow);
        int ih = oh + dh, iw = ow + dw;
        if (ih >= 0 && ih < aH && iw >= 0 && iw < aW) {
          if (aup) { ih >>= 1; iw >>= 1; }
          px = xbase + (unsigned)((((unsigned)n * Hs + ih) * Ws + iw) * aCin + r_off[i]);
        }
        py = ybase + (unsigned)((unsigned)m * aCout + r_off[i]);
      }
      glds16_asm(px, stage + (wave * 2 + i) * 1024);
      glds16_asm(py, stage + TILE + (wave * 2 + i) * 1024);
    }
    i_p0 += 32;
  };

  f32x4_t acc[4][4];   // [co tile][ci tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const bool do_bias = a.want_bias && tap == 0 && cit == 0 && wi == 0;     // see conv_mfma_wgrad3_kernel
  const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(H16_ONE_X2, H16_ONE_X2, H16_ONE_X2, H16_ONE_X2));
  f32x4_t accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) accb[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int KT = (int)((me - mb + 31) / 32);
  constexpr int INFLIGHT = (NS - 2) * 4;
#pragma unroll
  for (int t = 0; t < NS - 1; ++t)
    if (t < KT) issue(t);
  int buf = 0;
  for (int kt = 0; kt < KT; ++kt) {
    if (kt + NS - 2 < KT) wait_vmcnt<INFLIGHT>(); else wait_vmcnt<0>();
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (kt + NS - 1 < KT) {
      int nb = buf + NS - 1;
      if (nb >= NS) nb -= NS;
      issue(nb);
    }
    const unsigned char* Xb = smem + buf * STAGE;
    const unsigned char* Yb = Xb + TILE;
    bf16x8_t yf[4], xf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) yf[i] = frag_tr_swz(Yb, 0, wo * 8 + i * 2, lane, a.use_tr, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) xf[j] = frag_tr_swz(Xb, 0, wi * 8 + j * 2, lane, a.use_tr, a.relu_in);
    if (do_bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) accb[i] = mfma16(yf[i], ones, accb[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma16(yf[i], xf[j], acc[i][j]);
    if (++buf == NS) buf = 0;
  }
  float* slab = a.slab + (long)by * a.slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + wo * 64 + i * 16 + (lane >> 4) * 4;
      const int ci = ci0 + wi * 64 + j * 16 + (lane & 15);
      float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      *(float4*)(slab + ((long)tap * a.Cin + ci) * a.Cout + co) = v;
    }
  if (do_bias && (lane & 15) == 0) {
    float* bs = slab + (long)a.cells * a.Cin * a.Cout;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *(float4*)(bs + co0 + wo * 64 + i * 16 + (lane >> 4) * 4) = make_float4(accb[i][0], accb[i][1], accb[i][2], accb[i][3]);
  }
}

template <int NS>
__global__ __launch_bounds__(256) void conv_mfma_wgrad_glds_kernel(MfmaWgradArgs a) {
  wgrad_glds_body<NS>(a, blockIdx.x, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------
// filter gradient, three horizontal taps per workgroup (3x3 filters, W in {4,8,16,32}).
// The per-tap kernels above re-read every input and gradient pixel once per tap and channel tile
// (64 FLOP per byte fetched from L2) and sit on the L2->LDS bandwidth.  Here one workgroup owns
// (kh, 64 input channels, 128 output channels) and accumulates kw = 0,1,2 from the SAME staged rows:
// the tap shift is a +-1 row offset of the transposing LDS read, the left/right SAME-padding columns
// are removed by a loop-invariant AND mask on the input fragments (a stage is 32 consecutive pixels
// and W divides 32, so the column of fragment slot k is k mod W in every stage).  128 FLOP per byte.
//   stage: X rows = pixels p0-4 .. p0+35 (40 x 128 B, 8 rows per deposit), Y rows = p0 .. p0+31 (32 x 256 B)
//   waves 2 (ci) x 2 (co): wave tile 32 ci x 64 co x 3 taps = 24 MFMA accumulators (96 registers)
// ---------------------------------------------------------------------------------------------
// bias gradient = column sums of dy.  Extra workgroups (blockIdx.x >= number of filter tiles) stream ONLY the dy
// rows of their pixel chunk and multiply each transposed fragment with an all-ones operand on the matrix core.
// Kept as a separate code path so that its accumulators share registers with the filter path (occupancy).
template <int NS>
__device__ __forceinline__ void wgrad_bias_block(const MfmaWgradArgs& a, unsigned char* smem, int cot, long mb, long me, float* slab) {
  constexpr int YT = 32 * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int co0 = cot * 128;
  const int y_row0 = (wave * 2) * 4 + (lane >> 4), y_row1 = y_row0 + 4;
  const int y_c0 = co0 + ((lane & 15) ^ ((y_row0 & 7) << 1)) * 8;
  const int y_c1 = co0 + ((lane & 15) ^ ((y_row1 & 7) << 1)) * 8;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  long i_p0 = mb;
  const bf16_t* ady = a.dy; const bf16_t* azero = a.zero;
  int aCout = a.Cout;
  asm volatile("" : "+s"(ady), "+s"(azero), "+s"(aCout));        // (pinned in scalar registers: see wgrad3_body)
  auto issue = [&](int buf) {
    const unsigned stage = lds0 + buf * YT;
    const long m0 = i_p0 + y_row0, m1 = i_p0 + y_row1;
    const bf16_t* py0 = m0 < me ? ady + (unsigned)((unsigned)m0 * aCout + y_c0) : azero;
    const bf16_t* py1 = m1 < me ? ady + (unsigned)((unsigned)m1 * aCout + y_c1) : azero;
    glds16_asm(py0, stage + (wave * 2) * 1024);
    glds16_asm(py1, stage + (wave * 2 + 1) * 1024);
    i_p0 += 32;
  };
  int offy[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = g * 4 + (li >> 2);
    const int slot0 = wave * 4 + i * 2;
    offy[i] = row * 256 + (((slot0 + ((li & 3) >> 1)) ^ ((row & 7) << 1)) << 4) + (li & 1) * 8;
  }
  const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(H16_ONE_X2, H16_ONE_X2, H16_ONE_X2, H16_ONE_X2));
  f32x4_t accb[2] = {(f32x4_t){0.f, 0.f, 0.f, 0.f}, (f32x4_t){0.f, 0.f, 0.f, 0.f}};
  const int KT = (int)((me - mb + 31) / 32);
#pragma unroll
  for (int t = 0; t < NS - 1; ++t)
    if (t < KT) issue(t);
  for (int kt0 = 0; kt0 < KT; kt0 += NS) {
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      const int kt = kt0 + sidx;
      if (kt < KT) {
        if (kt + NS - 2 < KT) wait_vmcnt_any<(NS - 2) * 2>(); else wait_vmcnt_any<0>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + NS - 1 < KT) issue((sidx + NS - 1) % NS);
        const unsigned char* sb = smem + sidx * YT;
#pragma unroll
        for (int i = 0; i < 2; ++i)
          accb[i] = mfma16(tr_pair(sb + offy[i], 16 * 256), ones, accb[i]);
      }
    }
  }
  if ((lane & 15) == 0) {
    float* bs = slab + (long)a.cells * a.Cin * a.Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *(float4*)(bs + co0 + wave * 32 + i * 16 + (lane >> 4) * 4) = make_float4(accb[i][0], accb[i][1], accb[i][2], accb[i][3]);
  }
}

// timing-only ablations of the three-tap body (scripts/build_p8_ablate.sh w<k>; results are wrong by construction): 1 = no LDS-DMA after the
// prologue, 2 = no MFMAs, 4 = fragment reads of the first stage only, 8 = no ReLU / edge masks on the pixel fragments
#ifndef WG3_ABLATE
#define WG3_ABLATE 0
#endif

// SUB: the sub-pixel form (MfmaWgradArgs::sub != 0, checked by the caller): two column taps per workgroup (dw = tb, tb + 1 with
// tb = -1 or 0 by the column parity) instead of three -- 16 accumulators, the tap rows and the edge mask chosen once per workgroup
template <int NS, bool RELU, bool SUB>
__device__ __forceinline__ void wgrad3_body(const MfmaWgradArgs& a, const unsigned bx, const unsigned by) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int XT = 40 * 128, YT = 32 * 256, STAGE = XT + YT;
  constexpr int NT = SUB ? 2 : 3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave & 1, wo = wave >> 1;
  const int nci = a.Cin / 64, nco = a.Cout / 128;
  const long mb = (long)by * a.m_chunk;
  long me = mb + a.m_chunk;
  if (me > a.M) me = a.M;
  const int sub = SUB ? a.sub : 0;
  const int trows = SUB ? (sub == 3 ? 1 : 8) : a.KH;        // tile rows: filter rows kh, or (pa, pb, s) of the sub-pixel form
  if ((int)bx >= trows * nci * nco) {      // bias-gradient workgroup (only launched when want_bias)
    // (sub 1: dy lives on the full-resolution grid, whose pixels [4 mb, 4 me) are as good a quarter-share as any)
    wgrad_bias_block<NS>(a, smem, (int)bx - trows * nci * nco, sub == 1 ? 4 * mb : mb, sub == 1 ? 4 * me : me,
                         a.slab + (long)by * a.slab_stride);
    return;
  }
  int b = (int)bx;
  const int cot = b % nco; b /= nco;
  const int cit = b % nci; b /= nci;
  const int kh = b;
  const int ci0 = cit * 64, co0 = cot * 128;
  // The problem's geometry, PINNED in scalar registers (round 5).  `a` lives in the kernel-argument segment (a grouped launch indexes it with
  // the problem number) and the compiler re-read its fields there on every use: 17 s_load + 9 s_waitcnt lgkmcnt(0) in the address
  // arithmetic of EVERY K-step, each a scalar-cache round trip in front of the LDS-DMA issue.  An empty asm makes the copies opaque
  // (scripts/bench_wgrad_group.py: the critic's 32x32 layer alone 78.7 -> 70.9 us, the critic step's set 166 -> 155 us).
  const bf16_t* ax = a.x; const bf16_t* ady = a.dy; const bf16_t* azero = a.zero;
  int aH = a.H, aW = a.W, aCin = a.Cin, aCout = a.Cout, alw = a.lw, alh = a.lh;
  long aM = a.M;
  asm volatile("" : "+s"(ax), "+s"(ady), "+s"(azero), "+s"(aH), "+s"(aW), "+s"(aCin), "+s"(aCout), "+s"(alw), "+s"(alh), "+s"(aM));
  const int pa = kh >> 2, pb = (kh >> 1) & 1, srow = kh & 1;                 // sub-pixel form only
  const int dh = !SUB ? kh - a.PT : (sub == 3 ? 0 : (sub == 1 ? srow - 1 + pa : srow - pa));
  // first column tap: dw = tap - 1 for the three taps, or dw in {-1, 0} / {0, +1} by the column parity (1x1: dw = 0, second tap idle)
  const int tb = !SUB ? -1 : (sub == 3 ? 0 : ((sub == 1 ? pb == 0 : pb == 1) ? -1 : 0));
  const int ntap = (SUB && sub == 3) ? 1 : NT;
  const bool relu_on = RELU && a.relu_in;      // (a grouped launch is compiled for its 3x3 layers' flavour; a riding 1x1 may differ)
  const int g = lane >> 4, li = lane & 15;

  // ---- DMA roles -------------------------------------------------------------------------------
  // Y: deposits q = 2*wave + {0,1}; lane -> row q*4 + lane/16, 16-B slot lane%16
  const int y_row0 = (wave * 2) * 4 + (lane >> 4), y_row1 = y_row0 + 4;
  const int y_c0 = co0 + ((lane & 15) ^ ((y_row0 & 7) << 1)) * 8;
  const int y_c1 = co0 + ((lane & 15) ^ ((y_row1 & 7) << 1)) * 8;
  // X: deposit q = wave (and q = 4 from wave 0); lane -> row q*8 + lane/8, 16-B slot lane%8
  const int x_rowa = wave * 8 + (lane >> 3), x_rowb = 32 + (lane >> 3);
  const int x_ca = ci0 + ((lane & 7) ^ (((x_rowa >> 1) & 3) << 1)) * 8;        // (rows 32 + r share row r's swizzle key)
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

  // (pixel indices are 32-bit in the loop -- the element counts are bounded by the host -- : half the vector ALU work of 64-bit compares and adds)
  const int M32 = (int)aM;
  int i_p0 = (int)mb;
  // Linear addressing (round 5; the nearest-upsampled input, whose source row is floor(row / 2), goes to the per-tap kernel or, by default,
  // to the sub-pixel form sub = 1).  A K-step advances the reduction index by 32 pixels = whole grid
  // rows (W divides 32), so every lane's source address advances by the SAME amount per step, also in the strided sub-pixel forms (4 W elements
  // per grid row of the full-resolution tensor): dy is fetched through a scalar base that steps + a constant per-lane offset -- no vector ALU
  // work at all (chunks are whole K-steps: wgrad3_geom) --, x through a per-lane offset that steps, with the in-image test (halo rows
  // read the zero page) as two compares and a select instead of the pixel's decomposition, three multiplies and two divergent branches.
  auto y_lin = [&](int row) -> unsigned {        // element offset of pixel (step base + row), step base = a multiple of 32
    if (sub != 1) return (unsigned)(row * aCout);
    return (unsigned)((4 * aW * (row >> alw) + 2 * (row & (aW - 1)) + pa * 2 * aW + pb) * aCout);
  };
  auto x_lin = [&](int m, int coff) -> unsigned {      // element offset of the pixel tap row dh of reduction pixel m reads (m < 0: the same line, continued)
    if (sub == 2) return (unsigned)((4 * aW * (m >> alw) + 2 * (m & (aW - 1)) + (2 * dh + pa) * 2 * aW + pb) * aCin + coff);
    return (unsigned)((m + dh * aW) * aCin + coff);
  };
  const unsigned yv0 = 2u * (y_lin(y_row0) + (unsigned)y_c0), yv1 = 2u * (y_lin(y_row1) + (unsigned)y_c1);
  const bf16_t* ybase = ady + (sub == 1 ? 4L : 1L) * mb * aCout;
  const long ystep = (sub == 1 ? 128L : 32L) * aCout;
  // (wave 0's second x deposit, rows 32..39 of the stage, reads what its first one reads a K-step later: same lane pattern, same swizzle key)
  unsigned xoa = x_lin((int)mb - 4 + x_rowa, x_ca);
  const unsigned xstep = (sub == 2 ? 128u : 32u) * (unsigned)aCin;
  auto x_ptr = [&](int rowc, unsigned xo) -> const bf16_t* {
    const int m = i_p0 + rowc;
    const int ih = (int)__builtin_amdgcn_ubfe((unsigned)m, (unsigned)alw, (unsigned)alh) + dh;
    const bool ok = (unsigned)m < (unsigned)M32 && (unsigned)ih < (unsigned)aH;
    return ok ? ax + xo : azero;
  };
  auto issue = [&](int buf) {
    const unsigned stage = lds0 + buf * STAGE;
    glds16_sbase(ybase, yv0, stage + XT + (wave * 2) * 1024);
    glds16_sbase(ybase, yv1, stage + XT + (wave * 2 + 1) * 1024);
    ybase += ystep;
    glds16_asm(x_ptr(x_rowa - 4, xoa), stage + wave * 1024);
    xoa += xstep;
    if (wave == 0) glds16_asm(x_ptr(x_rowb - 4, xoa), stage + 4 * 1024);
    i_p0 += 32;
  };

  // ---- fragment addresses (per lane, stage-relative) and the left/right column masks -----------------
  // lane (g, li): channel = subtile*16 + li... transposing read: row = k-group g*4 + li/4, columns 4*(li%4)..+3
  int offx[NT][2], offy[4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = 4 + (t + tb) + g * 4 + (li >> 2);
      const int slot0 = wi * 4 + j * 2;
      offx[t][j] = row * 128 + (((slot0 + ((li & 3) >> 1)) ^ (((row >> 1) & 3) << 1)) << 4) + (li & 1) * 8;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = g * 4 + (li >> 2);
    const int slot0 = wo * 8 + i * 2;
    offy[i] = XT + row * 256 + (((slot0 + ((li & 3) >> 1)) ^ ((row & 7) << 1)) << 4) + (li & 1) * 8;
  }
  // fragment element e <-> pixel k = (e<4 ? g*4+e : 16+g*4+e-4); maskl clears the pixels of image column 0 (tap dw = -1),
  // maskr those of column W-1 (dw = +1).  SUB: only one of the two taps needs a mask -- mask1 belongs to tap 0 when tb = -1
  // (dw = -1: left) and to tap 1 when tb = 0 (dw = +1: right)
  uint32_t maskl[4], maskr[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t ml = 0, mr = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = 2 * d + h;
      const int k = (e < 4) ? (g * 4 + e) : (16 + g * 4 + (e - 4));
      const int ow = k & (a.W - 1);
      if (ow != 0) ml |= 0xFFFFu << (16 * h);
      if (ow != a.W - 1) mr |= 0xFFFFu << (16 * h);
    }
    maskl[d] = ml; maskr[d] = mr;
    if (SUB) { maskl[d] = tb < 0 ? ml : 0xFFFFFFFFu; maskr[d] = tb < 0 ? 0xFFFFFFFFu : mr; }     // = the masks of tap 0 / tap 1
  }

  f32x4_t acc[NT][4][2];   // [kw][co subtile][ci subtile]
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int KT = (int)((me - mb + 31) / 32);
#pragma unroll
  for (int t = 0; t < NS - 1; ++t)
    if (t < KT) issue(t);
  for (int kt0 = 0; kt0 < KT; kt0 += NS) {
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      const int kt = kt0 + sidx;
      if (kt < KT) {
        // this wave's share of stage kt has landed once at most (NS-2) newer stages are still in flight
        if (kt + NS - 2 < KT) {
          if (wave == 0) wait_vmcnt_any<(NS - 2) * 4>(); else wait_vmcnt_any<(NS - 2) * 3>();
        } else {
          wait_vmcnt_any<0>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + NS - 1 < KT && !(WG3_ABLATE & 1)) issue((sidx + NS - 1) % NS);
        const unsigned char* sb = smem + ((WG3_ABLATE & 4) ? 0 : sidx) * STAGE;
        bf16x8_t yf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) yf[i] = tr_pair(sb + offy[i], 16 * 256);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (SUB && t >= ntap) continue;        // (workgroup-uniform: the 1x1 form)
          bf16x8_t xf[2];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            uint4 v = __builtin_bit_cast(uint4, tr_pair(sb + offx[t][j], 16 * 128));
            if (!(WG3_ABLATE & 8)) {
            if (SUB ? relu_on : RELU) { v.x = relu_bf16x2(v.x); v.y = relu_bf16x2(v.y); v.z = relu_bf16x2(v.z); v.w = relu_bf16x2(v.w); }
            // (column 0 can only be fragment element 0 or 4, column W-1 only element 3 or 7 -- W divides the 4-pixel runs a lane holds:
            // the left mask lives in words 0 and 2, the right one in words 1 and 3)
            if (t == 0) { v.x &= maskl[0]; v.z &= maskl[2]; }
            if (t == NT - 1) { v.y &= maskr[1]; v.w &= maskr[3]; }
            }
            xf[j] = __builtin_bit_cast(bf16x8_t, v);
          }
          if (WG3_ABLATE & 2) {       // keep the fragment reads alive without the matrix pipe
#pragma unroll
            for (int j = 0; j < 2; ++j) asm volatile("" :: "v"(xf[j]));
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" :: "v"(yf[i]));
            continue;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[t][i][j] = mfma16(yf[i], xf[j], acc[t][i][j]);
        }
      }
    }
  }
  // D[row = co (4*(lane>>4)+r)][col = ci (lane&15)]
  float* slab = a.slab + (long)by * a.slab_stride;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (SUB && t >= ntap) continue;
    // slab cell: tap (kh, t), or [(pa*2 + pb)*4 + s*2 + d] with d = t, the rank among this parity's two taps
    const int cell = !SUB ? kh * 3 + t : (kh >> 1) * 4 + srow * 2 + t;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int co = co0 + wo * 64 + i * 16 + (lane >> 4) * 4;
        const int ci = ci0 + wi * 32 + j * 16 + (lane & 15);
        float4 v = make_float4(acc[t][i][j][0], acc[t][i][j][1], acc[t][i][j][2], acc[t][i][j][3]);
        *(float4*)(slab + ((long)cell * a.Cin + ci) * a.Cout + co) = v;
      }
  }
}


template <int NS, bool RELU>
__global__ __launch_bounds__(256) void conv_mfma_wgrad3_kernel(MfmaWgradArgs a) {
  if (__builtin_expect(a.sub != 0, 0)) wgrad3_body<NS, RELU, true>(a, blockIdx.x, blockIdx.y);
  else wgrad3_body<NS, RELU, false>(a, blockIdx.x, blockIdx.y);
}

// Several layers' filter gradients in ONE launch: workgroup b belongs to the problem p with first[p] <= b < first[p+1]
// and plays (b - first[p]) % gx[p], (b - first[p]) / gx[p] of that problem's own grid.  The 8x8 / 16x16 discriminator layers
// launch 224..602 workgroups each and are latency-bound alone; together their workgroups share the CUs (3 fit per CU).
// The image-end layers' filter gradients (conv_image.h: D.Block.1.Conv1 / Shortcut) ride in the same launch as its LAST
// img.first[IMG_GROUP_MAX] workgroups.  Alone they are two launches of a few hundred short workgroups plus two slab reductions
// (59 us per critic step, 4 % of the iteration); here ~128 workgroups per layer walk their pixel blocks in the CU slots the
// three-tap workgroups leave free and finish under them: 8.41 -> 8.19 ms per iteration.  Measured: leading instead of trailing
// workgroups +0.11 ms, 512 / 1024 instead of 128 per layer +0.19 / +0.46 ms (slots taken from the three-tap workgroups,
// more slabs), 32 per layer +0.38 ms (they outlast the launch).
struct WgradGroup {
  int n;
  int xcd_runs;             // consecutive three-tap workgroups (a pixel chunk's tiles) on one XCD
  unsigned first[WGRAD_GROUP_MAX + 1];
  unsigned gx[WGRAD_GROUP_MAX];
  MfmaWgradArgs a[WGRAD_GROUP_MAX];
  ImgWGroup img;
  HeadWgradRider head;      // the projection head's deferred parameter sums: head.blocks workgroups behind the image-end ones (three-tap launches only)
};
static_assert(sizeof(WgradGroup) <= 4096, "kernel argument block");

template <int NS, bool RELU>
__global__ __launch_bounds__(256) void conv_mfma_wgrad3_group_kernel(WgradGroup g) {
  // (the branch is marked unlikely so that its code is laid out BEHIND the three-tap body: with the image-end code in front the
  // same, instruction-for-instruction identical hot loop ran 40 % slower -- 198 vs 141 us for the critic step's eleven layers)
  unsigned b = blockIdx.x;
  if (__builtin_expect(b >= g.first[g.n], 0)) {         // the image-end workgroups trail the grid, the head's trail them
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_img[];
    const unsigned bb = b - g.first[g.n];
    if (bb >= g.img.first[IMG_GROUP_MAX]) head_wgrad_body(g.head.a, g.head.dEg, (int)(bb - g.img.first[IMG_GROUP_MAX]), (float*)smem_img);
    else img_wgrad_group_body(g.img, bb, smem_img);
    return;
  }
  // Workgroups are dealt to the 8 XCDs round-robin by blockIdx.  The workgroups of one pixel chunk (consecutive indices: the filter rows and
  // channel tiles of a layer) read the same dy and x pixels: run them on ONE XCD, through one L2 (round 4; RCGAN_WGRAD3_XCD=0 restores the
  // dealt order) -- dealt out, every XCD fetched every chunk: 1.3 GB from beyond L2 per launch of a 256-channel layer at ~6.7 TB/s
  if (g.xcd_runs) {
    const unsigned t8 = g.first[g.n] >> 3;
    if (b < t8 * 8) b = (b & 7) * t8 + (b >> 3);
  }
  int p = 0;
#pragma unroll
  for (int q = 1; q < WGRAD_GROUP_MAX; ++q)
    if (q < g.n && b >= g.first[q]) p = q;
  const unsigned l = b - g.first[p];
  const unsigned gxp = g.gx[p];
  // (the sub-pixel body behind the three-tap one, as the image-end body: see the note on code placement above)
  if (__builtin_expect(g.a[p].sub != 0, 0)) wgrad3_body<NS, RELU, true>(g.a[p], l % gxp, l / gxp);
  else wgrad3_body<NS, RELU, false>(g.a[p], l % gxp, l / gxp);
}

// the same grouping for the per-tap kernel (1x1 shortcuts and the shapes the three-tap kernel does not take)
template <int NS>
__global__ __launch_bounds__(256) void conv_mfma_wgrad_glds_group_kernel(WgradGroup g) {
  const unsigned b = blockIdx.x;
  if (__builtin_expect(b >= g.first[g.n], 0)) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_img[];
    img_wgrad_group_body(g.img, b - g.first[g.n], smem_img);
    return;
  }
  int p = 0;
#pragma unroll
  for (int q = 1; q < WGRAD_GROUP_MAX; ++q)
    if (q < g.n && b >= g.first[q]) p = q;
  const unsigned l = b - g.first[p];
  const unsigned gxp = g.gx[p];
  wgrad_glds_body<NS>(g.a[p], l % gxp, l / gxp);
}

// ---------------------------------------------------------------------------------------------
// slab reduction
// ---------------------------------------------------------------------------------------------
// out[i] (= or +=) sum_z slab[z][i]; the slabs may carry a bias-gradient tail of `nbias` floats after `count`
__global__ void slab_reduce2_kernel(const float* slab, long stride, float* out, long count, float* bias_out, int nbias, int nz,
                                    int accumulate) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count + nbias) return;
  float s = 0.f;
#pragma unroll 4
  for (int z = 0; z < nz; ++z) s += slab[(long)z * stride + i];
  float* o = i < count ? out + i : bias_out + (i - count);
  if (accumulate) s += *o;
  *o = s;
}

// the same reduction for several filter gradients in one launch (blockIdx.y = problem).  Slabs of the image-end kernels
// (conv_image.h: [32][Cb] + 32 floats per workgroup) are described by bias_off / orient: the bias sums sit at bias_off instead of
// behind the filter elements, and with orient 1 (the small side is dy) slab element k*Cb + n goes to dW[(t*Cb + n)*Cs + c],
// k = t*Cs + c.
#define REDUCE_GROUP_MAX 16
struct SlabReduceGroup {
  struct Item {
    const float* slab; long stride; float* out; long count; float* bias_out; int nbias, nz, accumulate;
    long bias_off;          // slab index of the first bias sum (= count for the three-tap / per-tap slabs)
    int orient, Cb, Cs;     // orient 1: transposed image-end mapping
    int sub;                // 1 / 2: the slab holds the 16 cells of the sub-pixel form (MfmaWgradArgs::sub), folded into the 9 taps here
    long cc;                // Cin * Cout (sub only)
    int bias_parts;         // 2: two bias partials per slab, nbias floats apart (the nine-tap kernel's upsample form); 0 / 1: one
    int vec4;               // a thread sums FOUR consecutive filter elements with 16-byte loads (count, cc, stride multiples of 4, orient 0)
  } it[REDUCE_GROUP_MAX];
};
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__global__ void slab_reduce2_group_kernel(SlabReduceGroup g) {
  const SlabReduceGroup::Item& r = g.it[blockIdx.y];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r.vec4) {
    // threads [0, count / 4): four elements each, the same per-element order of additions as the scalar form below (bit-identical sums);
    // threads behind them: the bias tail, one element each, through the scalar form
    const long nv = r.count >> 2;
    if (i < nv) {
      const long e = i << 2;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r.sub) {
        const int tap = (int)(e / r.cc), kh = tap / 3, kw = tap - kh * 3;
        const long rem = e - (long)tap * r.cc;
        long c4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int pa = q >> 1, pb = q & 1;
          const int sa = ((r.sub == 1) == (pa == 0)) ? (kh >= 1) : (kh >= 2);
          const int sb = ((r.sub == 1) == (pb == 0)) ? (kw >= 1) : (kw >= 2);
          c4[q] = (long)(q * 4 + sa * 2 + sb) * r.cc + rem;
        }
        int z = 0;
        for (; z + 2 <= r.nz; z += 2) {
          float4 v[2][4];
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[u][q] = *(const float4*)(r.slab + (long)(z + u) * r.stride + c4[q]);
#pragma unroll
          for (int u = 0; u < 2; ++u) s = f4add(s, f4add(f4add(v[u][0], v[u][1]), f4add(v[u][2], v[u][3])));
        }
        for (; z < r.nz; ++z) {
          const float* sl = r.slab + (long)z * r.stride;
          s = f4add(s, f4add(f4add(*(const float4*)(sl + c4[0]), *(const float4*)(sl + c4[1])), f4add(*(const float4*)(sl + c4[2]), *(const float4*)(sl + c4[3]))));
        }
        if (r.sub == 2) { s.x *= 0.25f; s.y *= 0.25f; s.z *= 0.25f; s.w *= 0.25f; }
      } else {
        int z = 0;
        for (; z + 8 <= r.nz; z += 8) {
          float4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(r.slab + (long)(z + u) * r.stride + e);
#pragma unroll
          for (int u = 0; u < 8; ++u) s = f4add(s, v[u]);
        }
#pragma unroll 4
        for (; z < r.nz; ++z) s = f4add(s, *(const float4*)(r.slab + (long)z * r.stride + e));
      }
      float4* o = (float4*)(r.out + e);
      if (r.accumulate) s = f4add(s, *o);
      *o = s;
      return;
    }
    i = r.count + (i - nv);       // a bias element (or past the end)
  }
  if (i >= r.count + r.nbias) return;
  const long si = i < r.count ? i : r.bias_off + (i - r.count);
  float s = 0.f;
  if (r.sub && i < r.count) {
    // dW[kh][kw] = scale * sum over the parities (pa, pb) of G[pa][pb][S(pa, kh)][S(pb, kw)]
    const int tap = (int)(i / r.cc), kh = tap / 3, kw = tap - kh * 3;
    const long rem = i - (long)tap * r.cc;
    long c4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pa = q >> 1, pb = q & 1;
      // S(sub 1): parity 0 -> 0,1,1; parity 1 -> 0,0,1.  S(sub 2): the other way round
      const int sa = ((r.sub == 1) == (pa == 0)) ? (kh >= 1) : (kh >= 2);
      const int sb = ((r.sub == 1) == (pb == 0)) ? (kw >= 1) : (kw >= 2);
      c4[q] = (long)(q * 4 + sa * 2 + sb) * r.cc + rem;
    }
    // (the loads of four slabs -- sixteen values -- are requested before the first of them is added: the loop is a chain of
    // memory round trips, not of additions)
    int z = 0;
    for (; z + 4 <= r.nz; z += 4) {
      float v[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[u][q] = r.slab[(long)(z + u) * r.stride + c4[q]];
#pragma unroll
      for (int u = 0; u < 4; ++u) s += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
    }
    for (; z < r.nz; ++z) {
      const float* sl = r.slab + (long)z * r.stride;
      s += (sl[c4[0]] + sl[c4[1]]) + (sl[c4[2]] + sl[c4[3]]);
    }
    if (r.sub == 2) s *= 0.25f;
  } else {
    int z = 0;
    for (; z + 16 <= r.nz; z += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = r.slab[(long)(z + u) * r.stride + si];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
#pragma unroll 4
    for (; z < r.nz; ++z) s += r.slab[(long)z * r.stride + si];
    if (i >= r.count && r.bias_parts == 2) {
#pragma unroll 4
      for (z = 0; z < r.nz; ++z) s += r.slab[(long)z * r.stride + si + r.nbias];
    }
  }
  float* o;
  if (i >= r.count) o = r.bias_out + (i - r.count);
  else if (r.orient == 0) o = r.out + i;
  else {
    const int k = (int)(i / r.Cb), n = (int)(i - (long)k * r.Cb);
    const int t = k / r.Cs, c = k - t * r.Cs;
    o = r.out + ((long)t * r.Cb + n) * r.Cs + c;
  }
  if (r.accumulate) s += *o;
  *o = s;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool mfma_wgrad_eligible(const rcgan_conv_desc* d) {
  return mfma_eligible(d) && d->cin % 128 == 0 && d->cout % 128 == 0;
}

static bool wgrad3_shape(int kh, int kw, int h, int w) {
  // three-taps-per-workgroup kernel: 3x3 filters, W a power of two dividing the 32-pixel stage, H a power of two
  return kh == 3 && kw == 3 && ilog2_exact(w) >= 0 && ilog2_exact(h) >= 0 && w >= 4 && w <= 32;
}

static bool wgrad3_geom(const MfmaWgradArgs& a) {     // (sub-pixel and 1x1 forms: the grid of the reduction index decides)
  if (a.M % 32 != 0 || a.up) return false;       // whole K-steps: the dy stream of the linear addressing has no tail test; no floor(row / 2) sources
  return a.sub ? wgrad3_shape(3, 3, a.H, a.W) : (wgrad3_shape(a.KH, a.KW, a.H, a.W) && a.PL == 1);
}

// RCGAN_WGRAD_IMPL (read once): unset = every kernel; "glds" = the per-tap kernels only; "reg" = only the register-staged per-tap kernel
enum { WGRAD_IMPL_ALL, WGRAD_IMPL_GLDS, WGRAD_IMPL_REG };
static int wgrad_impl() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("RCGAN_WGRAD_IMPL"); v = (e && e[0] == 'r') ? WGRAD_IMPL_REG : (e && e[0] == 'g') ? WGRAD_IMPL_GLDS : WGRAD_IMPL_ALL; }
  return v;
}

static long wgrad_clamp_splits(long want, long M) {
  static const int min_px = env_int("RCGAN_WGRAD_MINPX", 256);
  long maxs = (M + min_px - 1) / min_px;
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  if (want > 128) want = 128;
  return want;
}

// the three-tap kernel's tiles (rows: wgrad3_rows) and the pixel chunks of a layer ALONE on it
static long wgrad3_tiles(int rows, int cin, int cout) { return (long)rows * (cin / 64) * (cout / 128); }
static long wgrad3_alone_chunks(int rows, int cin, int cout, long M) {
  return wgrad_clamp_splits((WGRAD3_ALONE_WGS + wgrad3_tiles(rows, cin, cout) - 1) / wgrad3_tiles(rows, cin, cout), M);
}

// The pixel chunks a layer's slabs are sized for: the most that any kernel mfma_wgrad_choose may pick plans for it alone (sub, M: as posed)
int mfma_wgrad_splits(const rcgan_conv_desc* d, long M, int sub) {
  if (sub) return (int)wgrad3_alone_chunks(d->kh == 1 ? 1 : 8, d->cin, d->cout, M);
  long tiles = (long)d->kh * d->kw * (d->cin / 128) * (d->cout / 128);
  long want = wgrad_clamp_splits((WGRAD_TAP_ALONE_WGS + tiles - 1) / tiles, M);
  if (wgrad3_shape(d->kh, d->kw, d->h, d->w)) {
    want = std::max(want, wgrad3_alone_chunks(d->kh, d->cin, d->cout, M));
    // ... or the nine-tap kernel: one round of workgroups (a 256-channel layer: 8 tiles x 32 chunks, not the 22 of the rule above)
    const long tiles9 = (long)(d->cin / 64) * (d->cout / 128);
    if (d->cin % 64 == 0 && d->cout % 128 == 0) want = std::max(want, wgrad_clamp_splits((WGRAD9_ALONE_WGS + tiles9 - 1) / tiles9, M));
  }
  return (int)want;
}

// What rcgan_conv_workspace_bytes promises a matrix-core filter gradient: the slabs of the PLAIN pose on the full-resolution grid.  (The call
// checks mfma_wgrad_ws_need of its own pose -- the sub-pixel one: 16 cells per slab, chunks of the low-resolution grid --, not this promise.)
size_t mfma_wgrad_ws_bytes(const rcgan_conv_desc* d) {
  int oh, ow, p;
  same_pad(d->h, d->kh, d->stride, &oh, &p);
  same_pad(d->w, d->kw, d->stride, &ow, &p);
  const long M = (long)d->n * oh * ow;
  return mfma_wgrad_ws_need(mfma_wgrad_splits(d, M, 0), ((size_t)d->kh * d->kw * d->cin + 1) * d->cout, M, d->cout) + 256;
}

// Sub-pixel filter gradient (MfmaWgradArgs::sub) of an upsample-3x3 (1) or ConvMeanPool (2) layer: 0 where the layer is posed
// as an ordinary 3x3 filter gradient (shape the three-tap kernel does not take, RCGAN_WGRAD_SUBPIXEL=0)
int mfma_wgrad_sub_kind(const rcgan_conv_desc* d, int use_tr) {
  static const int on = env_int("RCGAN_WGRAD_SUBPIXEL", 1);
  if (!use_tr || wgrad_impl() != WGRAD_IMPL_ALL || !mfma_wgrad_eligible(d)) return 0;
  if (d->kh == 1 && d->kw == 1) {
    // a SMALL 1x1 (the down blocks' shortcuts: 0.27 GFLOP at the bench batch) rides in the grouped launch on the two-tap body; a big
    // one keeps the per-tap kernel's 128 x 128 tiles (a staged pixel feeds one tap's MFMAs here: a third of the arithmetic intensity)
    static const double max_gflop = env_int("RCGAN_WGRAD_1X1_GROUP_MAXMFLOP", 600) * 1e6;
    const double fl = 2.0 * d->n * d->h * d->w * (double)d->cin * d->cout;
    // (the reduction index runs in whole 32-pixel K-steps: wgrad3_geom)
    return fl <= max_gflop && !(d->flags & (RCGAN_CONV_OUT_MEANPOOL2 | RCGAN_CONV_IN_UPSAMPLE2X)) && wgrad3_shape(3, 3, d->h, d->w) &&
           ((long)d->n * d->h * d->w) % 32 == 0 ? 3 : 0;
  }
  if (!on || d->kh != 3 || d->kw != 3) return 0;
  const bool up = (d->flags & RCGAN_CONV_IN_UPSAMPLE2X) != 0, pool = (d->flags & RCGAN_CONV_OUT_MEANPOOL2) != 0;
  if (up == pool || (d->h & 1) || (d->w & 1)) return 0;
  if (!wgrad3_shape(3, 3, d->h / 2, d->w / 2) || ((long)d->n * (d->h / 2) * (d->w / 2)) % 32 != 0) return 0;
  return up ? 1 : 2;
}

template <bool RELU>
static int launch_wgrad3(rcgan_ctx* ctx, MfmaWgradArgs& a, dim3 grid) {
  constexpr int NS = 4;
  static bool attr = false;
  size_t lds = (size_t)NS * (40 * 128 + 32 * 256);
  if (!attr) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_mfma_wgrad3_kernel<NS, RELU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  {
    ProfScope ps(ctx, RCGAN_PROF_WGRAD_MFMA, 2.0 * (double)a.M * wgrad3_alg_taps(a) * a.Cin * a.Cout,
                 2.0 * (double)a.M * wgrad3_exec_taps(a) * a.Cin * a.Cout);
    hipLaunchKernelGGL((conv_mfma_wgrad3_kernel<NS, RELU>), grid, dim3(256), lds, ctx->stream, a);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

template <bool GLDS>      // the per-tap kernels: direct-to-LDS or register-staged
static int launch_wgrad_tap(rcgan_ctx* ctx, const MfmaWgradArgs& a, dim3 grid) {
  constexpr int NS = 4;
  const void* kernel = GLDS ? (const void*)conv_mfma_wgrad_glds_kernel<NS> : (const void*)conv_mfma_wgrad_kernel;
  const size_t lds = GLDS ? (size_t)NS * 2 * 32 * 256 : (size_t)4 * 64 * WG_PITCH * sizeof(bf16_t);
  static bool attr = false;
  if (!attr) {
    RC_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  {
    ProfScope ps(ctx, RCGAN_PROF_WGRAD_MFMA, 2.0 * (double)a.M * a.KH * a.KW * a.Cin * a.Cout);
    if constexpr (GLDS) hipLaunchKernelGGL(conv_mfma_wgrad_glds_kernel<NS>, grid, dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(conv_mfma_wgrad_kernel, grid, dim3(256), lds, ctx->stream, a);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// THE choice of a filter-gradient kernel for a posed problem: the only holder of the precedence nine-tap > three-tap > per-tap direct-to-LDS >
// per-tap register-staged, the only reader of RCGAN_WGRAD_IMPL (wgrad_impl) and of RCGAN_WGRAD9_MINWORK; mfma_wgrad_launch and the group
// planner (rcgan_conv2d_bwd_weight_group) launch what it returns.  nine: how the nine-tap kernel is on offer (WgradNine).
int mfma_wgrad_choose(rcgan_ctx* ctx, const MfmaWgradArgs& a, WgradNine nine, WgradKernel* k) {
  const bool three = wgrad_impl() == WGRAD_IMPL_ALL && a.use_tr && a.zero != nullptr && wgrad3_geom(a);
  if (a.sub && !three) RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "sub-pixel filter gradient needs the three-tap kernel");
  if (nine == WGRAD9_BY_WORK) {
    // the nine-tap kernel where a workgroup's share of the pixels amortises its nine-cell slab (scripts/bench_conv.py, n = 128, layers alone:
    // 32x32 256-channel 175 -> 142 us, 32x32 128-channel 72 -> 67, 16x16 256-channel 60 -> 60; but 8x8 256-channel 32 -> 37, 8x8 128-channel
    // 21 -> 28, the sub-pixel forms 43 -> 83 / 122 -> 128: those stay on the three-tap kernel)
    const long min_work = env_int("RCGAN_WGRAD9_MINWORK", 200000);        // (read per call: the tests force the kernel on small shapes)
    const long work9 = a.M * (long)(a.Cin / 64) * (a.Cout / 128);
    nine = (a.sub ? min_work <= 0 : work9 >= min_work) ? WGRAD9_ON : WGRAD9_OFF;
  }
  *k = nine == WGRAD9_ON && mfma_wgrad9_takes(a) ? WK_NINE : three ? WK_THREE
     : wgrad_impl() != WGRAD_IMPL_REG && a.zero != nullptr ? WK_TAP_GLDS : WK_TAP_REG;
  return RCGAN_OK;
}

// THE plan of problem p.a on kernel k: pixel chunk, slab stride and grid of gx tiles x gy <= nz pixel chunks.  px_per_block > 0 (three- and
// nine-tap kernel in a group): the caller fixes the pixels per workgroup for all layers (equal workgroup run times, far fewer fp32 slabs to write
// and reduce); 0: chunks for WGRAD*_ALONE_WGS workgroups.  The per-tap kernels take the nz chunks the slabs were sized for, alone or grouped.
void mfma_wgrad_plan(MfmaWgradPlanned& p, WgradKernel k, int nz, long px_per_block) {
  MfmaWgradArgs& a = p.a;
  if (k == WK_NINE) return mfma_wgrad9_plan(p, nz, px_per_block);
  long want = nz;
  p.gx = (unsigned)(a.KH * a.KW * (a.Cin / 128) * (a.Cout / 128));
  if (k == WK_THREE) {
    want = px_per_block > 0 ? wgrad_clamp_splits(cdiv(a.M, px_per_block), a.M) : wgrad3_alone_chunks(wgrad3_rows(a), a.Cin, a.Cout, a.M);
    if (want > nz) want = nz;
    if (want < 1) want = 1;
    p.gx = (unsigned)(wgrad3_tiles(wgrad3_rows(a), a.Cin, a.Cout) + (a.want_bias ? a.Cout / 128 : 0));
  }
  a.m_chunk = ((a.M + want - 1) / want + 63) / 64 * 64;
  a.slab_stride = wgrad_slab_floats(a, 1);
  p.gy = (unsigned)cdiv(a.M, a.m_chunk);
}

// One layer alone: choose, plan, check the planned slabs against the workspace, launch.  Returns the number of slabs written (a: as planned).
int mfma_wgrad_launch(rcgan_ctx* ctx, MfmaWgradArgs& a, int nz, bool* bias_done, size_t ws_bytes) {
  *bias_done = false;
  WgradKernel k;
  int rc = mfma_wgrad_choose(ctx, a, WGRAD9_BY_WORK, &k);
  if (rc) return rc;
  MfmaWgradPlanned p = {a, 0, 0};
  mfma_wgrad_plan(p, k, nz, 0);
  const auto fits = [&] { return (size_t)p.gy * (size_t)p.a.slab_stride * sizeof(float) <= ws_bytes; };
  if (k == WK_NINE && !fits()) {       // (its upsample form carries two bias tails per slab: more than the stride the caller sized for)
    rc = mfma_wgrad_choose(ctx, a, WGRAD9_OFF, &k);
    if (rc) return rc;
    mfma_wgrad_plan(p, k, nz, 0);
  }
  if (!fits()) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "planned slabs need %zu have %zu", (size_t)p.gy * p.a.slab_stride * sizeof(float), ws_bytes);
  a = p.a;
  const dim3 grid(p.gx, p.gy);
  rc = k == WK_NINE ? mfma_wgrad9_group_launch(ctx, 1, &p)
     : k == WK_THREE ? (a.relu_in ? launch_wgrad3<true>(ctx, a, grid) : launch_wgrad3<false>(ctx, a, grid))
     : k == WK_TAP_GLDS ? launch_wgrad_tap<true>(ctx, a, grid) : launch_wgrad_tap<false>(ctx, a, grid);
  *bias_done = a.want_bias != 0 && k != WK_TAP_REG;
  return rc ? rc : (int)p.gy;
}

template <bool RELU>
static int launch_wgrad3_group(rcgan_ctx* ctx, const WgradGroup& g) {
  constexpr int NS = 4;
  static bool attr = false;
  size_t lds = (size_t)NS * (40 * 128 + 32 * 256);
  if (!attr) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_mfma_wgrad3_group_kernel<NS, RELU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  double fl = 0, fx = 0;
  for (int p = 0; p < g.n; ++p) {
    fl += 2.0 * (double)g.a[p].M * wgrad3_alg_taps(g.a[p]) * g.a[p].Cin * g.a[p].Cout;
    fx += 2.0 * (double)g.a[p].M * wgrad3_exec_taps(g.a[p]) * g.a[p].Cin * g.a[p].Cout;
  }
  {
    ProfScope ps(ctx, RCGAN_PROF_WGRAD_MFMA, fl, fx);
    hipLaunchKernelGGL((conv_mfma_wgrad3_group_kernel<NS, RELU>), dim3(g.img.first[IMG_GROUP_MAX] + g.first[g.n] + g.head.blocks), dim3(256), lds, ctx->stream, g);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

static int launch_wgrad_glds_group(rcgan_ctx* ctx, const WgradGroup& g) {
  constexpr int NS = 4;
  static bool attr = false;
  size_t lds = (size_t)NS * 2 * 32 * 256;
  if (!attr) {
    RC_HIP(ctx, hipFuncSetAttribute((const void*)conv_mfma_wgrad_glds_group_kernel<NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  double fl = 0;
  for (int p = 0; p < g.n; ++p) fl += 2.0 * (double)g.a[p].M * g.a[p].KH * g.a[p].KW * g.a[p].Cin * g.a[p].Cout;
  {
    ProfScope ps(ctx, RCGAN_PROF_WGRAD_MFMA, fl);
    hipLaunchKernelGGL(conv_mfma_wgrad_glds_group_kernel<NS>, dim3(g.img.first[IMG_GROUP_MAX] + g.first[g.n]), dim3(256), lds, ctx->stream, g);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// probs[i] planned (mfma_wgrad_plan) for the three-tap kernel (family 0; all with the same relu_in) or the per-tap direct-to-LDS kernel (family 1)
// img (optional): image-end problems that ride in the FIRST launch
int mfma_wgrad3_group_launch(rcgan_ctx* ctx, int n, const MfmaWgradPlanned* probs, int family, const ImgWGroup* img, bool carry_head) {
  static_assert(ImgWGeom<128>::LDS <= 4 * (40 * 128 + 32 * 256), "image-end body needs more LDS than the three-tap kernel");
  static_assert((HEAD_MAX_V + 1) * HEAD_MAX_D * 4 <= 4 * (40 * 128 + 32 * 256), "head body needs more LDS than the three-tap kernel");
  for (int i0 = 0; i0 < n; i0 += WGRAD_GROUP_MAX) {
    WgradGroup g;
    static const int xcd_runs = env_int("RCGAN_WGRAD3_XCD", 1);
    g.xcd_runs = xcd_runs;
    g.head.blocks = 0;
    if (carry_head && family != 1 && i0 == 0) (void)head_take_wgrad(ctx, &g.head);
    if (img && i0 == 0) g.img = *img;
    else { g.img.n = 0; for (int q = 0; q <= IMG_GROUP_MAX; ++q) g.img.first[q] = 0; }
    g.n = (n - i0 < WGRAD_GROUP_MAX) ? n - i0 : WGRAD_GROUP_MAX;
    unsigned tot = 0;
    for (int p = 0; p < g.n; ++p) {
      g.a[p] = probs[i0 + p].a;
      g.gx[p] = probs[i0 + p].gx;
      g.first[p] = tot;
      tot += probs[i0 + p].gx * probs[i0 + p].gy;
    }
    for (int p = g.n; p <= WGRAD_GROUP_MAX; ++p) g.first[p] = tot;
    for (int p = g.n; p < WGRAD_GROUP_MAX; ++p) { g.gx[p] = 1; g.a[p] = probs[i0].a; }
    int rc = family == 1 ? launch_wgrad_glds_group(ctx, g)
                         : (probs[i0].a.relu_in ? launch_wgrad3_group<true>(ctx, g) : launch_wgrad3_group<false>(ctx, g));
    if (rc) return rc;
  }
  return RCGAN_OK;
}

extern "C" {

// The matrix-core filter-gradient problem of a layer (everything but the slab) and the number of pixel chunks its slabs are sized for.
// Upsample-3x3 and ConvMeanPool layers the three-tap kernel takes are posed in their sub-pixel form (MfmaWgradArgs::sub): reduction over
// the low-resolution grid.
static int wgrad_pose(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, bool want_bias, MfmaWgradArgs& a, int* nz) {
  int oh, ow, pt, pl;
  same_pad(d->h, d->kh, 1, &oh, &pt);
  same_pad(d->w, d->kw, 1, &ow, &pl);
  a.x = (const bf16_t*)x; a.dy = (const bf16_t*)dy; a.slab = nullptr;
  a.zero = (const bf16_t*)ctx->zero_page;
  a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cout = d->cout; a.KH = d->kh; a.KW = d->kw; a.PT = pt; a.PL = pl;
  a.up = (d->flags & RCGAN_CONV_IN_UPSAMPLE2X) ? 1 : 0;
  a.relu_in = (d->flags & RCGAN_CONV_IN_RELU) ? 1 : 0;
  a.use_tr = g_use_tr;
  a.sub = mfma_wgrad_sub_kind(d, g_use_tr);
  if ((d->flags & RCGAN_CONV_OUT_MEANPOOL2) && a.sub != 2)
    RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "filter gradient from the pooled dy needs the sub-pixel three-tap kernel (rcgan_conv_wgrad_pool_ok)");
  if (a.sub == 1 || a.sub == 2) { a.H >>= 1; a.W >>= 1; a.up = 0; }
  a.cells = (a.sub == 1 || a.sub == 2) ? 16 : d->kh * d->kw;
  a.M = (long)d->n * a.H * a.W;
  a.lw = ilog2_exact(a.W); a.lh = ilog2_exact(a.H);
  if (a.lw < 0 || a.lh < 0) { a.lw = -1; a.lh = -1; }
  a.slab_stride = wgrad_slab_floats(a, 1);
  a.want_bias = want_bias ? 1 : 0;
  a.m_chunk = 0;
  *nz = mfma_wgrad_splits(d, a.M, a.sub);
  return RCGAN_OK;
}

static SlabReduceGroup::Item wgrad_reduce_item(const rcgan_conv_desc* d, const MfmaWgradArgs& a, float* dw, float* dbias, int nbias, int nz, int accumulate) {
  SlabReduceGroup::Item it = {};
  it.slab = a.slab; it.stride = a.slab_stride; it.out = dw; it.count = (long)d->kh * d->kw * d->cin * d->cout;
  it.bias_out = dbias; it.nbias = nbias; it.nz = nz; it.accumulate = accumulate;
  it.bias_off = (long)a.cells * d->cin * d->cout;
  it.sub = a.sub == 3 ? 0 : a.sub; it.cc = (long)d->cin * d->cout;
  it.bias_parts = a.slab_stride == it.bias_off + 2L * d->cout ? 2 : 1;       // (mfma_wgrad9_plan's upsample form)
  static const int vec4_on = [] { const char* e = getenv("RCGAN_SLAB_REDUCE_VEC4"); return e ? atoi(e) : 1; }();
  it.vec4 = vec4_on && it.count % 4 == 0 && it.cc % 4 == 0 && a.slab_stride % 4 == 0 && ((size_t)a.slab & 15) == 0 && ((size_t)dw & 15) == 0;
  return it;
}

// One launch of slab_reduce2_group_kernel for the m <= REDUCE_GROUP_MAX items at `items`, on grid_x x m workgroups (the unused slots of the
// argument block repeat the first item)
static int slab_reduce_group_launch(rcgan_ctx* ctx, const SlabReduceGroup::Item* items, int m, int grid_x) {
  SlabReduceGroup g;
  for (int q = 0; q < REDUCE_GROUP_MAX; ++q) g.it[q] = items[q < m ? q : 0];
  hipLaunchKernelGGL(slab_reduce2_group_kernel, dim3(grid_x, m), dim3(256), 0, ctx->stream, g);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_conv_wgrad_pool_ok(const rcgan_conv_desc* d) {
  // (before the self test has run the transposing LDS read counts as available; rcgan_conv2d_bwd_weight re-checks)
  return d && (d->flags & RCGAN_CONV_OUT_MEANPOOL2) && mfma_wgrad_sub_kind(d, g_use_tr < 0 ? 1 : g_use_tr) == 2 ? 1 : 0;
}

int rcgan_conv2d_bwd_weight(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias,
                            int accumulate, void* ws, size_t ws_bytes) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  if (mfma_wgrad_eligible(d)) {
    rc = ensure_selftest(ctx);
    if (rc) return rc;
    MfmaWgradArgs a;
    int nz = 0;
    rc = wgrad_pose(ctx, d, x, dy, dbias != nullptr, a, &nz);
    if (rc) return rc;
    a.slab = (float*)ws;
    long cnt = (long)d->kh * d->kw * d->cin * d->cout;
    size_t need = mfma_wgrad_ws_need(nz, a.slab_stride, a.M, d->cout);
    if (ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
    bool bias_done = false;
    int nzz = mfma_wgrad_launch(ctx, a, nz, &bias_done, ws_bytes);
    if (nzz < 0) return nzz;
    const int nb = bias_done ? d->cout : 0;
    if (a.sub == 1 || a.sub == 2) {
      const SlabReduceGroup::Item it = wgrad_reduce_item(d, a, dw, dbias, nb, nzz, accumulate);
      rc = slab_reduce_group_launch(ctx, &it, 1, cdiv(cnt + nb, 256));
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL(slab_reduce2_kernel, dim3(cdiv(cnt + nb, 256)), dim3(256), 0, ctx->stream, (const float*)a.slab, a.slab_stride, dw, cnt,
                         dbias, nb, nzz, accumulate);
      RC_LAUNCH_CHECK(ctx);
    }
    if (dbias && !bias_done) {
      float* part = (float*)((char*)ws + (size_t)nz * a.slab_stride * sizeof(float));
      rc = colsum_launch<bf16_t>(ctx, (const bf16_t*)dy, a.M, d->cout, dbias, accumulate, part);
      if (rc) return rc;
    }
    return RCGAN_OK;
  }
  return conv_wgrad_off_mfma(ctx, d, x, dy, dw, dbias, accumulate, ws, ws_bytes);
}

// The family (vector of planned problems) among fam[0, nfam) whose launch has the most workgroups; -1 if none qualifies.  Only the first
// `counted` problems of a family count; skip_empty: a family without problems is no candidate; later_wins_ties: >= instead of >.
static int wgrad_busiest_family(const std::vector<MfmaWgradPlanned>* fam, int nfam, size_t counted, bool skip_empty, bool later_wins_ties) {
  int best_f = -1;
  unsigned best = 0;
  for (int f = 0; f < nfam; ++f) {
    if (skip_empty && fam[f].empty()) continue;
    unsigned tot = 0;
    for (size_t q = 0; q < fam[f].size() && q < counted; ++q) tot += fam[f][q].gx * fam[f][q].gy;
    if (best_f < 0 || (later_wins_ties ? tot >= best : tot > best)) { best = tot; best_f = f; }
  }
  return best_f;
}

// What rcgan_conv2d_bwd_weight_group has decided about its layers (wgrad_group_plan) before anything is launched (wgrad_group_issue)
struct WgradGroupPlan {
  std::vector<MfmaWgradPlanned> fam9[4];         // nine-tap kernel: plain without / with input ReLU, sub-pixel forms without / with
  std::vector<MfmaWgradPlanned> fam[3];          // three-tap kernel without / with input ReLU (the riding 1x1 layers among them), per-tap kernel
  ImgWGroup img;                                 // image-end layers: they ride in the first launch of family img_f (if there is one) and in the grouped reduction
  int img_f = -1, head_f = -1;                   // the families whose first launch carries the image-end workgroups / the projection head's deferred sums
  std::vector<SlabReduceGroup::Item> red;        // what the grouped reductions sum
  std::vector<int> own;                          // the layers that get a call of their own, in layer order
  size_t used = 0;                               // bytes of the first workspace half that the grouped slabs take
};

// Which kernel each layer gets, the pixels per workgroup of the three- and nine-tap families, where each slab lies in the first workspace
// half, which family the riders join, which layers fall back to a call of their own, what the reductions sum.  Launches nothing (but the
// one-off self test of ensure_selftest).
static int wgrad_group_plan(rcgan_ctx* ctx, int n, const rcgan_conv_desc* descs, const void* const* xs, const void* const* dys,
                            float* const* dws, float* const* dbiases, int accumulate, void* ws, size_t ws_bytes, WgradGroupPlan& plan) {
  static const int target_blocks = [] { const char* e = getenv("RCGAN_WGRAD_GROUP_BLOCKS"); return e ? atoi(e) : 448; }();      // (512 before the sub-pixel forms: 6.67 -> 6.64 ms with 384; round 4, the critic step's launch with its chunks' workgroups on one XCD and the generator step's big layers gone to the nine-tap kernel, same box: 384 5.65 ms, 448 5.59, 512 5.60, 576 5.75)
  struct Cand { MfmaWgradArgs a = {}; int nz = 0; WgradKernel k = WK_TAP_REG; };      // (WK_TAP_REG: not grouped -- no matrix-core layer, or that kernel)
  std::vector<Cand> cand(n);
  // The nine-tap kernel (conv_wgrad9.hip) takes the group's 3x3 layers when they are big: its one workgroup per CU writes a slab of ALL nine
  // (sixteen) cells, and the riders of the three-tap launch (image-end layers, 1x1 shortcuts, the head) lose the workgroups they hid under.
  // Measured on the bench iteration: the critic step's layers (n = 128, 128 channels: 1152 pixels per workgroup) 120 -> 172 us with it, the
  // generator step's (256 channels: 12032 / 2560 pixels per workgroup) 478 -> 425 us.
  const long w9_minwork = [] { const char* e = getenv("RCGAN_WGRAD9_GROUP_MINWORK"); return e ? atol(e) : 1000000L; }();      // (per call: the tests force it; the critic step's group is 0.52 M, the generator step's 2.75 M, one 256-channel 32x32 layer 1.05 M)
  bool wgrad9_group_on = false;
  {
    double w9 = 0;
    for (int i = 0; i < n; ++i) {
      const rcgan_conv_desc* d = descs + i;
      if (check_desc(ctx, d) || !mfma_wgrad_eligible(d) || d->kh != 3) continue;
      w9 += (double)d->n * d->h * d->w * (d->cin / 64) * (d->cout / 128);       // (full-resolution pixels x channel tiles)
    }
    wgrad9_group_on = w9 >= (double)w9_minwork;
  }
  // pass 1: which layers the grouped kernel takes, and the pixels per workgroup that gives ~target_blocks workgroups in all
  double work = 0, work9[2] = {0, 0};        // (work9: the nine-tap kernel's plain / sub-pixel layers, one workgroup per CU each)
  for (int i = 0; i < n; ++i) {
    const rcgan_conv_desc* d = descs + i;
    int rc = check_desc(ctx, d);
    if (rc) return rc;
    if (!mfma_wgrad_eligible(d)) continue;
    rc = ensure_selftest(ctx);
    if (rc) return rc;
    MfmaWgradArgs& a = cand[i].a;
    rc = wgrad_pose(ctx, d, xs[i], dys[i], dbiases[i] != nullptr, a, &cand[i].nz);
    if (rc) return rc;
    rc = mfma_wgrad_choose(ctx, a, wgrad9_group_on ? WGRAD9_ON : WGRAD9_OFF, &cand[i].k);
    if (rc) return rc;
    if (cand[i].k == WK_NINE) {
      work9[a.sub ? 1 : 0] += (double)a.M * (a.Cin / 64) * (a.Cout / 128) * (a.sub ? 2 : 1);
    } else if (cand[i].k == WK_THREE) {
      // workgroup-passes over a pixel: 3 filter rows of three taps, or 8 (parity, row shift) tiles of two taps
      work += (double)a.M * (a.sub == 3 ? 1.0 / 3.0 : (a.sub ? 8 * 2.0 / 3.0 : a.KH)) * (a.Cin / 64) * (a.Cout / 128);
    }
  }
  static const int px_max = [] { const char* e = getenv("RCGAN_WGRAD_GROUP_PXMAX"); return e ? atoi(e) : 6144; }();
  long px = (long)(work / target_blocks);
  px = (px + 63) / 64 * 64;
  if (px < 256) px = 256;
  if (px > px_max) px = px_max;      // big groups (the generator step): more workgroups rather than ever longer ones
  static const int target9 = [] { const char* e = getenv("RCGAN_WGRAD9_BLOCKS"); return e ? atoi(e) : 256; }();
  // one workgroup per CU and equal pixels per workgroup: the smallest chunk with which the layers' tiles x chunks fit ONE round of target9
  // workgroups (a 257th workgroup would double the launch's time); the plain and the sub-pixel layers are a launch each
  long px9[2] = {0, 0};
  for (int f = 0; f < 2; ++f) {
    px9[f] = ((long)(work9[f] / target9) + 127) / 128 * 128;
    if (px9[f] < 512) px9[f] = 512;
    for (int it = 0; it < 4096 && work9[f] > 0; ++it, px9[f] += 128) {
      long tot = 0;
      for (int i = 0; i < n; ++i)
        if (cand[i].k == WK_NINE && (cand[i].a.sub != 0) == (f != 0)) {
          MfmaWgradPlanned b = {cand[i].a, 0, 0};
          mfma_wgrad_plan(b, WK_NINE, 1 << 20, px9[f]);
          tot += (long)b.gx * b.gy;
        }
      if (tot <= target9) break;
    }
  }
  // pass 2: slabs, the families of the grouped launches per input-ReLU flavour, everything else on its own
  auto& fam9 = plan.fam9;
  auto& fam = plan.fam;
  std::vector<MfmaWgradPlanned> late;            // small 1x1 layers on the two-tap body: join one of the first two
  auto& red = plan.red;
  size_t& used = plan.used;
  ImgWGroup& img = plan.img;
  img.n = 0;
  for (int q = 0; q <= IMG_GROUP_MAX; ++q) img.first[q] = 0;
  static const int img_group = [] { const char* e = getenv("RCGAN_WGRAD_GROUP_IMG"); return e ? atoi(e) : 1; }();
  bool any_group = false;
  for (int i = 0; i < n && img_group; ++i) any_group = any_group || cand[i].k == WK_THREE;
  for (int i = 0; i < n; ++i) {
    const rcgan_conv_desc* d = descs + i;
    bool grouped = false;
    if (any_group && img.n < IMG_GROUP_MAX && img_side(d) && (d->cin <= 3 ? d->cout : d->cin) == 128) {
      ImgWArgs ia;
      int cb = 0, nwg = 0;
      static const int img_wgs = [] { const char* e = getenv("RCGAN_WGRAD_IMG_WGS"); return e ? atoi(e) : 128; }();       // (with 384 three-tap workgroups: 6.64 -> 6.62 ms with 96; round 5, the three-tap workgroups a quarter faster: 96 5.36 ms, 128 5.34, 160 5.40, 256 5.36)
      int rc = img_wgrad_plan(ctx, d, xs[i], dys[i], img_wgs, &ia, &cb, &nwg);
      if (rc) return rc;
      const long per = 32L * cb + 32;
      const size_t need = ((size_t)nwg * per * sizeof(float) + 255) / 256 * 256;
      if (used + need <= ws_bytes / 2) {
        ia.slab = (float*)((char*)ws + used);
        used += need;
        const int q = img.n++;
        img.a[q] = ia;
        for (int r = q + 1; r <= IMG_GROUP_MAX; ++r) img.first[r] = img.first[q] + (unsigned)nwg;
        const int side = img_side(d), cs = side == 1 ? d->cin : d->cout, T = d->kh * d->kw;
        SlabReduceGroup::Item it = {};
        it.slab = ia.slab; it.stride = per; it.out = dws[i]; it.count = (long)T * cs * cb; it.nz = nwg; it.accumulate = accumulate;
        it.Cb = cb; it.Cs = cs;
        if (side == 1) {           // small = conv input: slab order is dW order; bias gradient = the ones row (31)
          it.orient = 0; it.bias_out = dbiases[i]; it.nbias = dbiases[i] ? cb : 0; it.bias_off = 31L * cb;
        } else {                   // small = dy: transposed; bias gradient = column sums of the centre tap
          it.orient = 1; it.bias_out = dbiases[i]; it.nbias = dbiases[i] ? cs : 0; it.bias_off = 32L * cb + (T == 9 ? 4 : 0) * cs;
        }
        red.push_back(it);
        grouped = true;
      }
    }
    const WgradKernel k = cand[i].k;
    if (!grouped && k != WK_TAP_REG) {
      MfmaWgradPlanned p = {cand[i].a, 0, 0};
      MfmaWgradArgs& a = p.a;
      // (the grouped slabs are fitted into the workspace below: no a-priori bound on the nine-tap kernel's pixel chunks)
      if (k == WK_NINE) mfma_wgrad_plan(p, k, 1 << 20, px9[a.sub ? 1 : 0]);
      else mfma_wgrad_plan(p, k, cand[i].nz, px);
      const size_t need = ((size_t)p.gy * a.slab_stride * sizeof(float) + 255) / 256 * 256;
      if (used + need <= ws_bytes / 2) {
        a.slab = (float*)((char*)ws + used);
        used += need;
        if (k == WK_NINE) fam9[(a.sub ? 2 : 0) + (a.relu_in ? 1 : 0)].push_back(p);
        else if (k == WK_THREE && a.sub == 3 && !a.relu_in) late.push_back(p);       // placed below
        else fam[k == WK_THREE ? (a.relu_in ? 1 : 0) : 2].push_back(p);
        red.push_back(wgrad_reduce_item(d, a, dws[i], dbiases[i], dbiases[i] ? d->cout : 0, (int)p.gy, accumulate));
        grouped = true;
      }
    }
    if (!grouped) plan.own.push_back(i);
  }
  // Three riders each hide under the family of grouped launches with the most workgroups.  Their rules differ, and the differences decide
  // which launch a rider lengthens (the bench iteration's timings were taken with exactly these): do not unify them.
  // * a riding 1x1 without input ReLU runs on either flavour of the three-tap kernel (the ReLU is a per-problem switch in the two-tap
  //   body): every planned problem counts, it may open a family of its own (an empty one is a candidate), and a tie stays with family 0
  if (!late.empty()) {
    const int f = wgrad_busiest_family(fam, 2, (size_t)-1, false, false);
    fam[f].insert(fam[f].end(), late.begin(), late.end());
  }
  // * the image-end workgroups ride in a family's FIRST launch (mfma_wgrad3_group_launch: WGRAD_GROUP_MAX problems) -- deliberately only
  //   those count and the family must exist; a tie goes to the later one, and the per-tap family (2) is a candidate
  int& img_f = plan.img_f;
  if (img.n) {
    img_f = wgrad_busiest_family(fam, 3, WGRAD_GROUP_MAX, true, true);
    RC_REQUIRE(ctx, img_f >= 0, "image-end filter gradients planned without a grouped launch");
  }
  // * the projection head's deferred parameter sums (head_rider.h) need a three-tap launch (families 0, 1): they follow the image-end
  //   workgroups there, else the same rule over those two
  if (ctx->head_stage == 2) plan.head_f = (img_f == 0 || img_f == 1) ? img_f : wgrad_busiest_family(fam, 2, WGRAD_GROUP_MAX, true, true);
  return RCGAN_OK;
}

// The launches of a plan in their stream order: the layers on their own (with the workspace half the grouped slabs do not use), the nine-tap
// families, the three-tap / per-tap families (riders in the first launch of theirs), the grouped reductions.
static int wgrad_group_issue(rcgan_ctx* ctx, const WgradGroupPlan& plan, const rcgan_conv_desc* descs, const void* const* xs,
                             const void* const* dys, float* const* dws, float* const* dbiases, int accumulate, void* ws, size_t ws_bytes) {
  for (int i : plan.own) {
    int rc = rcgan_conv2d_bwd_weight(ctx, descs + i, xs[i], dys[i], dws[i], dbiases[i], accumulate, (char*)ws + ws_bytes / 2, ws_bytes - ws_bytes / 2);
    if (rc) return rc;
  }
  for (int f = 0; f < 4; ++f)
    if (!plan.fam9[f].empty()) {
      int rc = mfma_wgrad9_group_launch(ctx, (int)plan.fam9[f].size(), plan.fam9[f].data());
      if (rc) return rc;
    }
  for (int f = 0; f < 3; ++f)
    if (!plan.fam[f].empty()) {
      // (the head's sums are taken from the context -- head_take_wgrad, head_stage 2 -> 0 -- when that launch is built)
      int rc = mfma_wgrad3_group_launch(ctx, (int)plan.fam[f].size(), plan.fam[f].data(), f == 2 ? 1 : 0, f == plan.img_f ? &plan.img : nullptr,
                                        f == plan.head_f);
      if (rc) return rc;
    }
  const std::vector<SlabReduceGroup::Item>& red = plan.red;
  for (size_t i0 = 0; i0 < red.size(); i0 += REDUCE_GROUP_MAX) {
    const int m = (int)((red.size() - i0 < REDUCE_GROUP_MAX) ? red.size() - i0 : REDUCE_GROUP_MAX);
    long maxc = 0;
    for (int q = 0; q < m; ++q) {
      const long threads = (red[i0 + q].vec4 ? red[i0 + q].count / 4 : red[i0 + q].count) + red[i0 + q].nbias;
      if (threads > maxc) maxc = threads;
    }
    int rc = slab_reduce_group_launch(ctx, &red[i0], m, cdiv(maxc, 256));
    if (rc) return rc;
  }
  return RCGAN_OK;
}

// Filter gradients of several layers whose x / dy are all available (the end of a backward pass): the layers the
// three-tap matrix-core kernel takes run as ONE grouped launch per input-ReLU flavour + ONE grouped slab reduction; every
// other layer goes through rcgan_conv2d_bwd_weight as usual.  Planned in full before the first launch: a failure while planning leaves
// nothing of the call on the stream.
int rcgan_conv2d_bwd_weight_group(rcgan_ctx* ctx, int n, const rcgan_conv_desc* descs, const void* const* xs, const void* const* dys,
                                  float* const* dws, float* const* dbiases, int accumulate, void* ws, size_t ws_bytes) {
  RC_REQUIRE(ctx, n >= 0 && (n == 0 || (descs && xs && dys && dws && dbiases)), "null argument");
  WgradGroupPlan plan;
  int rc = wgrad_group_plan(ctx, n, descs, xs, dys, dws, dbiases, accumulate, ws, ws_bytes, plan);
  return rc ? rc : wgrad_group_issue(ctx, plan, descs, xs, dys, dws, dbiases, accumulate, ws, ws_bytes);
}

// What rcgan_conv2d_bwd_weight_group needs at most: the call splits ws in two halves -- the second serves every layer that is computed by a
// call of its own (rcgan_conv_workspace_bytes of the largest), the first holds the slabs of the grouped launches (a layer whose slabs do
// not fit there is computed on its own instead: same values).  Each half: the largest single need plus the single needs of the layers
// that can be grouped (matrix-core and image-end layers), every term rounded up to 256 bytes.
size_t rcgan_conv2d_bwd_weight_group_workspace_bytes(int n, const rcgan_conv_desc* descs) {
  if (n <= 0 || descs == nullptr) return 0;
  size_t largest = 0, slabs = 0;
  for (int i = 0; i < n; ++i) {
    const rcgan_conv_desc* d = descs + i;
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->cin < 1 || d->cout < 1 || d->kh < 1 || d->kw < 1 || d->stride < 1) return 0;
    const size_t one = (rcgan_conv_workspace_bytes(d) + 255) / 256 * 256;
    largest = std::max(largest, one);
    if (mfma_wgrad_eligible(d) || img_side(d)) slabs += one;
  }
  return 2 * (largest + slabs);
}

}  // extern "C"
