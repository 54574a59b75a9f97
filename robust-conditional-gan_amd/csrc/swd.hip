// Sliced Wasserstein distance on Laplacian-pyramid patch descriptors (swd.py; Karras et al. 2018, section 5): the four device
// primitives.  Definition (restated in float64 by tests/swd_ref.py): images uint8 NHWC, c 1 or 3, h, w each 28 or 32.
//   G0 = x, G1 = down(G0), G2 = down(G1);  L0 = G0 - up(G1), L1 = G1 - up(G2), L2 = G2        (sizes 32/16/8 or 28/14/7 per side)
//   down: the taps [1,4,6,4,1]/16 along each axis, mirror boundary without repeating the edge (-1 -> 1, -2 -> 2, n -> n-2, n+1 -> n-3),
//         the even indices kept;  up: zero-insert to twice the size (u[2i,2j] = g[i,j]), then [1,4,6,4,1]/8 along each axis, same boundary.
// A level's descriptors are its 7 x 7 x c neighbourhoods centred on the lattice y = 3, 3 + stride, ... <= s_h - 4 (likewise x), n_pos of
// them per image, elements in the order (dy, dx, channel).  Per segment of images and per channel they are normalised with the mean
// and the standard deviation (ddof 0) of that channel over ALL descriptor entries of the segment (a pixel counts once per descriptor
// that covers it); a channel without deviation contributes 0.
//
// swd_image_moments / swd_segment_moments (rcgan_swd_moments): per image the fp64 sums of w v and w v^2 over the level's pixels v of a
// channel, w = the number of descriptors covering the pixel (every thread adds its pixels in fp64, a butterfly per wavefront, the
// four wavefronts in order); per segment the images' sums (thread t adds images lo + t, lo + t + 256, ..., then the same tree).
// swd_project (rcgan_swd_project): one workgroup of 256 threads walks images blockIdx.x, blockIdx.x + gridDim.x, ...; thread t keeps
// direction t % nd (nd <= 128 per launch) in 49 c registers and takes the positions t / nd, t / nd + 256 / nd, ...  Per image: sixteen-
// byte loads into LDS, the pyramid, the level normalised in place, the dot products (the level's values are LDS broadcasts), the
// nd x n_pos results staged in LDS and written as runs of n_pos floats.
// LDS (floats): h w c (G0) + h w c / 2 (a separable pass's intermediate) + h w c / 4 (G1) + h w c / 16 (G2) + 128 * 49 (stage) + 16:
// 46.3 KiB at 32 x 32 x 3, 30.1 KiB at 28 x 28 x 1 (the moments: without the stage, 21.8 KiB at most).
//
// Arithmetic and its bound (u = 2^-24).  Pixels are integers below 256.  down() of G0 forms multiples of 2^-8 below 256 (16 bits), of
// G1 multiples of 2^-16 (24 bits); up(G1) multiples of 2^-14, so L0 has 22 bits: all exact in fp32 in any order of summation.
// up(G2) is not: each of its two passes is a chain of at most three fused multiply-adds on non-negative values (the unnormalised
// partial sums stay below 8 * 255, the division by 8 is exact), at most 3 u 255 of error per pass, the second pass carrying the
// first one's error on with weights that sum to 1; the subtraction G1 - up(G2) rounds once more, |L1| <= 255.  Hence
//     |level value computed - exact| <= delta_l,    delta_0 = delta_2 = 0,   delta_1 = 7 u 255 = 1.07e-4.
// The moments are fp64 sums of exactly widened fp32 values, at most ~70 roundings deep: the mean mu' = S / N is within
// delta_l + 2^-40 of the exact mean mu and, sigma being 1-Lipschitz in the sup norm of its data, the deviation from the one-pass
// variance Q / N - mu'^2 has the relative error delta_l / sigma + eps64, eps64 = 2^-45 (Q / N) / sigma^2.  With r = 1 / sigma, both
// rounded to fp32 (relative u each), a level value becomes t = fl(v' - mu_f), xhat' = fl(t r_f):
//     |t - (v - mu)| <= a_l = 2 delta_l + 255 u + 510 u + 2^-40          (|mu| <= 255, |v - mu| <= 510)
//     |xhat' - xhat| <= r a_l + |xhat| (delta_l r + 2 u + eps64)          (to first order; delta_l r <= 1e-3 is assumed)
// and the dot product with the direction w (49 c fused multiply-adds in fp32, |w|_2 <= 1 + u so sum_i |w_i| <= sqrt(49 c) (1 + u))
// errs by gamma_{49c} sum_i |xhat'_i w_i|.  Together, for every entry of proj, with r_max the largest r of the segment's channels,
//     |proj - exact| <= (1 + 1e-5) (r_max a_l sqrt(49 c) + (delta_l r_max + (49 c + 2) u / (1 - 49 c u) + eps64) sum_i |xhat_i w_i|)
// (tests/swd_ref.py: ``projection_bound``; the test asserts exactly this).  A channel whose variance comes out <= 0 has r = 0: a
// channel that is constant over a segment has integer (L2) or exactly zero (L0, L1) level values, whose moments are exact.
//
// sort_local / sort_global (rcgan_sort_rows_f32): bitonic on the keys bits ^ (sign ? ~0 : 1 << 31), a total order (-0 before +0, +inf
// behind every finite value, nans outermost).  sort_local holds a chunk of min(width, 8192) keys in LDS (32 KiB) and runs every
// compare-exchange stride below the chunk; one launch of sort_global per stride at or above it.  Passes meet only at kernel
// boundaries.  absdiff_rowsum: one workgroup per row, fp64, the order fixed as above.
#include <math.h>

#include "common.h"
#include "seg_rows.h"

#pragma clang fp contract(off)     // (the fused operations are the ones written as fmaf: the error analysis above counts them)

#define SWD_THREADS 256
#define SWD_PATCH 7
#define SWD_MAX_POS 49
#define SWD_MAX_ND 128               // directions per launch of swd_project
#define SWD_SORT_CHUNK 8192          // keys a workgroup of sort_local holds
#define SWD_MISC 16                  // ints in front of the planes: the segment found, mean / rstd per channel

struct SwdPlan {
  int h, w, c, level, stride;
  int lh, lw, ny, nx, n_pos;         // the level's size, its lattice
};

static bool swd_plan(int h, int w, int c, int level, int stride, SwdPlan* p) {
  if (!((h == 28 || h == 32) && (w == 28 || w == 32) && (c == 1 || c == 3) && level >= 0 && level <= 2 && stride >= 1)) return false;
  p->h = h; p->w = w; p->c = c; p->level = level; p->stride = stride;
  p->lh = h >> level; p->lw = w >> level;
  p->ny = (p->lh - SWD_PATCH) / stride + 1;
  p->nx = (p->lw - SWD_PATCH) / stride + 1;
  p->n_pos = p->ny * p->nx;
  return p->n_pos <= SWD_MAX_POS;
}

static size_t swd_lds_floats(const SwdPlan& p) { const size_t e = (size_t)p.h * p.w * p.c; return SWD_MISC + e + e / 2 + e / 4 + e / 16; }

__device__ __forceinline__ int swd_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// dst [H/2][W/2][c] = down(src [H][W][c]); tmp holds [H][W/2][c].  Exact in fp32 for the two uses above.
__device__ void swd_down(const float* src, float* tmp, float* dst, int H, int W, int c) {
  const int Wo = W / 2, Ho = H / 2;
  for (int t = threadIdx.x; t < H * Wo * c; t += SWD_THREADS) {
    const int ch = t % c, xo = (t / c) % Wo, y = t / (c * Wo);
    const float* r = src + y * W * c + ch;
    const int x = 2 * xo;
    tmp[t] = ((r[swd_mirror(x - 2, W) * c] + r[swd_mirror(x + 2, W) * c]) + 4.f * (r[swd_mirror(x - 1, W) * c] + r[swd_mirror(x + 1, W) * c]) +
              6.f * r[x * c]) * 0.0625f;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Ho * Wo * c; t += SWD_THREADS) {
    const int q = t % (Wo * c), yo = t / (Wo * c), y = 2 * yo, S = Wo * c;
    dst[t] = ((tmp[swd_mirror(y - 2, H) * S + q] + tmp[swd_mirror(y + 2, H) * S + q]) +
              4.f * (tmp[swd_mirror(y - 1, H) * S + q] + tmp[swd_mirror(y + 1, H) * S + q]) + 6.f * tmp[y * S + q]) * 0.0625f;
  }
  __syncthreads();
}

// big [2H][2W][c] -= up(src [H][W][c]); tmp holds [H][2W][c].  Each pass: at most three fused multiply-adds, then the exact * 1/8.
__device__ void swd_sub_up(const float* src, float* tmp, float* big, int H, int W, int c) {
  const float k[5] = {1.f, 4.f, 6.f, 4.f, 1.f};
  const int W2 = 2 * W, H2 = 2 * H;
  for (int t = threadIdx.x; t < H * W2 * c; t += SWD_THREADS) {
    const int ch = t % c, X = (t / c) % W2, y = t / (c * W2);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int idx = swd_mirror(X + j - 2, W2);
      if (!(idx & 1)) acc = fmaf(k[j], src[(y * W + (idx >> 1)) * c + ch], acc);
    }
    tmp[t] = acc * 0.125f;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < H2 * W2 * c; t += SWD_THREADS) {
    const int q = t % (W2 * c), Y = t / (W2 * c);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int idx = swd_mirror(Y + j - 2, H2);
      if (!(idx & 1)) acc = fmaf(k[j], tmp[(idx >> 1) * W2 * c + q], acc);
    }
    big[t] = big[t] - acc * 0.125f;
  }
  __syncthreads();
}

// image `img` -> the plan's Laplacian level in LDS, [lh][lw][c]; returns where it lies.  planes: h w c * 29 / 16 floats.
__device__ float* swd_level(const SwdPlan& P, const uint8_t* __restrict__ img, float* planes) {
  const int e = P.h * P.w * P.c;
  float* g0 = planes;
  float* tmp = g0 + e;
  float* g1 = tmp + e / 2;
  float* g2 = g1 + e / 4;
  for (int q = threadIdx.x; q < e / 16; q += SWD_THREADS) {          // (e is a multiple of 16 for every admitted shape, img 16-byte aligned)
    const uint4 v = ((const uint4*)img)[q];
    const unsigned word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) g0[16 * q + b] = (float)((word[b >> 2] >> (8 * (b & 3))) & 255u);
  }
  __syncthreads();
  swd_down(g0, tmp, g1, P.h, P.w, P.c);
  if (P.level == 0) {
    swd_sub_up(g1, tmp, g0, P.h / 2, P.w / 2, P.c);
    return g0;
  }
  swd_down(g1, tmp, g2, P.h / 2, P.w / 2, P.c);
  if (P.level == 1) {
    swd_sub_up(g2, tmp, g1, P.h / 4, P.w / 4, P.c);
    return g1;
  }
  return g2;
}

__device__ __forceinline__ double swd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// six per-thread doubles -> their workgroup sums in out[0..6) (global), butterfly per wavefront, the four wavefronts in order
__device__ void swd_block_sum6(double* acc, double* red /* [4][6] LDS */, int count, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double s = swd_wave_sum(acc[k]);
    if (lane == 0) red[wave * 6 + k] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < count) out[threadIdx.x] = (red[threadIdx.x] + red[6 + threadIdx.x]) + (red[12 + threadIdx.x] + red[18 + threadIdx.x]);
}

__global__ __launch_bounds__(SWD_THREADS) void swd_image_moments_kernel(SwdPlan P, const uint8_t* __restrict__ x, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float swd_smem[];
  __shared__ double red[24];
  __shared__ int cover[64];                                            // descriptors covering row y: cover[y]; column x: cover[32 + x]
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int pos = tid & 31, size = tid < 32 ? P.lh : P.lw, count = tid < 32 ? P.ny : P.nx;
    int k = 0;
    for (int q = 0; q < count; ++q) k += (pos >= q * P.stride && pos < q * P.stride + SWD_PATCH && pos < size) ? 1 : 0;
    cover[tid] = k;
  }
  const float* lvl = swd_level(P, x + (size_t)blockIdx.x * (P.h * P.w * P.c), swd_smem + SWD_MISC);      // (ends in a barrier)
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (int t = tid; t < P.lh * P.lw; t += SWD_THREADS) {
    const double wgt = (double)(cover[t / P.lw] * cover[32 + t % P.lw]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      if (ch < P.c) {
        const double v = (double)lvl[t * P.c + ch];
        acc[2 * ch] += wgt * v;
        acc[2 * ch + 1] += wgt * (v * v);
      }
  }
  swd_block_sum6(acc, red, 2 * P.c, part + (size_t)blockIdx.x * 2 * P.c);
}

__global__ __launch_bounds__(SWD_THREADS) void swd_segment_moments_kernel(int n, int c, const int32_t* __restrict__ off, const double* __restrict__ part,
                                                                          double* __restrict__ mom) {
  __shared__ double red[24];
  int lo, hi;
  knn_segment(off, blockIdx.x, n, &lo, &hi);
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (int i = lo + threadIdx.x; i < hi; i += SWD_THREADS) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k < 2 * c) acc[k] += part[(size_t)i * 2 * c + k];
  }
  swd_block_sum6(acc, red, 2 * c, mom + (size_t)blockIdx.x * 2 * c);
}

// proj[d][s][e] = +inf for every e at or behind the segment's descriptor count
__global__ __launch_bounds__(SWD_THREADS) void swd_pad_kernel(int n, int n_pos, int n_seg, int width, const int32_t* __restrict__ off,
                                                              float* __restrict__ proj) {
  int lo, hi;
  knn_segment(off, blockIdx.x % n_seg, n, &lo, &hi);
  const long long have = (long long)(hi - lo) * n_pos;
  const int e = blockIdx.y * SWD_THREADS * 16 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int q = e + k * SWD_THREADS;
    if (q < width && q >= have) proj[(size_t)blockIdx.x * width + q] = __builtin_inff();
  }
}

template <int C>
__global__ __launch_bounds__(SWD_THREADS) void swd_project_kernel(SwdPlan P, int n, int n_seg, int d0, int nd, int width,
                                                                  const uint8_t* __restrict__ x, const int32_t* __restrict__ off,
                                                                  const double* __restrict__ mom, const float* __restrict__ dirs,
                                                                  float* __restrict__ proj) {
  extern __shared__ __attribute__((aligned(16))) float swd_smem[];
  int* found = (int*)swd_smem;                                         // [0]: the image's segment
  float* norm = swd_smem + 4;                                          // [2 ch]: mean, [2 ch + 1]: 1 / deviation
  float* planes = swd_smem + SWD_MISC;
  float* stage = planes + (P.h * P.w * C) / 16 * 29;                   // (behind G0, the intermediate, G1 and G2)
  const int tid = threadIdx.x, d = tid % nd, grp = tid / nd, groups = SWD_THREADS / nd;
  constexpr int D = SWD_PATCH * SWD_PATCH * C, ROW = SWD_PATCH * C;
  float wr[D];
  if (grp < groups) {
#pragma unroll
    for (int i = 0; i < D; ++i) wr[i] = dirs[(size_t)(d0 + d) * D + i];
  } else {
#pragma unroll
    for (int i = 0; i < D; ++i) wr[i] = 0.f;
  }
  for (int img = blockIdx.x; img < n; img += gridDim.x) {
    __syncthreads();                                                   // (the last image's stage and misc words have been read)
    if (tid == 0) found[0] = 0x7fffffff;
    __syncthreads();
    for (int s = tid; s < n_seg; s += SWD_THREADS) {
      int lo, hi;
      knn_segment(off, s, n, &lo, &hi);
      if (img >= lo && img < hi) atomicMin(found, s);                  // (an integer minimum: the lowest segment that holds the image)
    }
    __syncthreads();
    const int seg = found[0];
    if (seg == 0x7fffffff) continue;                                   // (the whole workgroup: an image outside every segment)
    int lo, hi;
    knn_segment(off, seg, n, &lo, &hi);
    if (tid < C) {
      const double N = (double)(hi - lo) * (double)(P.n_pos * SWD_PATCH * SWD_PATCH);
      const double mu = mom[((size_t)seg * C + tid) * 2] / N, var = mom[((size_t)seg * C + tid) * 2 + 1] / N - mu * mu;
      norm[2 * tid] = (float)mu;
      norm[2 * tid + 1] = var > 0. ? (float)(1. / sqrt(var)) : 0.f;
    }
    float* lvl = swd_level(P, x + (size_t)img * (P.h * P.w * C), planes);                                  // (ends in a barrier)
    for (int t = tid; t < P.lh * P.lw * C; t += SWD_THREADS) {
      const int ch = t % C;
      const float centred = lvl[t] - norm[2 * ch];
      lvl[t] = centred * norm[2 * ch + 1];
    }
    __syncthreads();
    if (grp < groups) {
      for (int p = grp; p < P.n_pos; p += groups) {
        const int py = p / P.nx, px = p - py * P.nx;
        const float* patch = lvl + ((py * P.stride) * P.lw + px * P.stride) * C;
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < SWD_PATCH; ++dy) {
          const float* row = patch + dy * P.lw * C;
#pragma unroll
          for (int j = 0; j < ROW; ++j) acc = fmaf(row[j], wr[dy * ROW + j], acc);
        }
        stage[d * P.n_pos + p] = acc;
      }
    }
    __syncthreads();
    const long long first = (long long)(img - lo) * P.n_pos;
    for (int t = tid; t < nd * P.n_pos; t += SWD_THREADS) {
      const int dd = t / P.n_pos, pp = t - dd * P.n_pos;
      if (first + pp < width) proj[((size_t)(d0 + dd) * n_seg + seg) * width + first + pp] = stage[t];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ the sort
__device__ __forceinline__ uint32_t swd_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t swd_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

// Chunk blockIdx.x (cw keys, cw a power of two that divides width) of the rows laid end to end: the stages k = k_first, 2 k_first,
// ..., k_last of the bitonic network, stage k_first from stride j_first down, every later one from k / 2 down, all strides < cw.
__global__ __launch_bounds__(SWD_THREADS) void swd_sort_local_kernel(uint32_t* __restrict__ x, int width, int cw, int k_first, int k_last, int j_first) {
  __shared__ uint32_t key[SWD_SORT_CHUNK];
  const size_t base = (size_t)blockIdx.x * cw;
  const int in_row = (int)(base & (size_t)(width - 1));
  for (int t = threadIdx.x; t < cw; t += SWD_THREADS) key[t] = swd_key(x[base + t]);
  __syncthreads();
  for (int k = k_first; k <= k_last && k > 0; k <<= 1) {
    for (int j = k == k_first ? j_first : k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < cw / 2; t += SWD_THREADS) {
        const int i = 2 * t - (t & (j - 1));
        const uint32_t a = key[i], b = key[i + j];
        const bool up = ((in_row + i) & k) == 0;
        if ((a > b) == up) { key[i] = b; key[i + j] = a; }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < cw; t += SWD_THREADS) x[base + t] = swd_unkey(key[t]);
}

// one compare-exchange pass of stage k at stride j over all rows (j < width: a pair never leaves its row)
__global__ __launch_bounds__(SWD_THREADS) void swd_sort_global_kernel(uint32_t* __restrict__ x, size_t pairs, int width, int k, int j) {
  const size_t t = (size_t)blockIdx.x * SWD_THREADS + threadIdx.x;
  if (t >= pairs) return;
  const size_t i = 2 * t - (t & (size_t)(j - 1));
  const uint32_t a = x[i], b = x[i + j];
  const bool up = (((int)(i & (size_t)(width - 1))) & k) == 0;
  if ((swd_key(a) > swd_key(b)) == up) { x[i] = b; x[i + j] = a; }
}

__global__ __launch_bounds__(SWD_THREADS) void swd_absdiff_rowsum_kernel(int width, int n_seg, const int32_t* __restrict__ count,
                                                                         const float* __restrict__ a, const float* __restrict__ b,
                                                                         double* __restrict__ out) {
  __shared__ double red[24];
  const int m = min(max(count[blockIdx.x % n_seg], 0), width);
  const float* pa = a + (size_t)blockIdx.x * width;
  const float* pb = b + (size_t)blockIdx.x * width;
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (int i = threadIdx.x; i < m; i += SWD_THREADS) acc[0] += fabs((double)pa[i] - (double)pb[i]);
  swd_block_sum6(acc, red, 1, out + blockIdx.x);
}

static bool swd_pow2(int v) { return v >= 1 && (v & (v - 1)) == 0; }

extern "C" {

int rcgan_swd_moments(rcgan_ctx* ctx, int n, int h, int w, int c, int level, int stride, int n_seg, const uint8_t* x, const int32_t* off,
                      double* part, double* mom) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  SwdPlan plan;
  const bool ok = swd_plan(h, w, c, level, stride, &plan) && n >= 1 && n_seg >= 1 && n_seg <= KNN_MAX_SEG && x && off && part && mom &&
                  ((uintptr_t)x & 15) == 0 && ((uintptr_t)off & 3) == 0 && ((uintptr_t)part & 7) == 0 && ((uintptr_t)mom & 7) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d (>= 1), h %d, w %d (28 or 32), c %d (1 or 3), level %d (0..2), stride %d (>= 1, at most %d positions), n_seg %d (1..%d), "
             "x (16-byte aligned) / off / part / mom %s", n, h, w, c, level, stride, SWD_MAX_POS, n_seg, KNN_MAX_SEG,
             x && off && part && mom ? "given" : "NULL");
  hipLaunchKernelGGL(swd_image_moments_kernel, dim3(n), dim3(SWD_THREADS), sizeof(float) * swd_lds_floats(plan), ctx->stream, plan, x, part);
  RC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(swd_segment_moments_kernel, dim3(n_seg), dim3(SWD_THREADS), 0, ctx->stream, n, c, off, (const double*)part, mom);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_swd_project(rcgan_ctx* ctx, int n, int h, int w, int c, int level, int stride, int n_seg, const uint8_t* x, const int32_t* off,
                      const double* mom, int n_dir, const float* dirs, int width, float* proj) {
  SwdPlan plan;
  const bool ok = swd_plan(h, w, c, level, stride, &plan) && n >= 1 && n_seg >= 1 && n_seg <= KNN_MAX_SEG && n_dir >= 1 && n_dir <= 1024 &&
                  swd_pow2(width) && (long long)n_dir * n_seg <= 0x7fffffffLL && x && off && mom && dirs && proj && ((uintptr_t)x & 15) == 0 &&
                  ((uintptr_t)off & 3) == 0 && ((uintptr_t)mom & 7) == 0 && ((uintptr_t)dirs & 3) == 0 && ((uintptr_t)proj & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d (>= 1), h %d, w %d (28 or 32), c %d (1 or 3), level %d (0..2), stride %d (>= 1, at most %d positions), n_seg %d (1..%d), "
             "n_dir %d (1..1024), width %d (a power of two), x (16-byte aligned) / off / mom / dirs / proj %s", n, h, w, c, level, stride, SWD_MAX_POS,
             n_seg, KNN_MAX_SEG, n_dir, width, x && off && mom && dirs && proj ? "given" : "NULL");
  hipLaunchKernelGGL(swd_pad_kernel, dim3(n_dir * n_seg, cdiv(width, SWD_THREADS * 16)), dim3(SWD_THREADS), 0, ctx->stream, n, plan.n_pos, n_seg, width,
                     off, proj);
  RC_LAUNCH_CHECK(ctx);
  const size_t lds = sizeof(float) * (swd_lds_floats(plan) + SWD_MAX_ND * SWD_MAX_POS);
  const int grid = n < 4 * ctx->num_cus ? n : 4 * ctx->num_cus;
  for (int d0 = 0; d0 < n_dir; d0 += SWD_MAX_ND) {
    const int nd = n_dir - d0 < SWD_MAX_ND ? n_dir - d0 : SWD_MAX_ND;
    if (c == 1)
      hipLaunchKernelGGL(swd_project_kernel<1>, dim3(grid), dim3(SWD_THREADS), lds, ctx->stream, plan, n, n_seg, d0, nd, width, x, off, mom, dirs, proj);
    else
      hipLaunchKernelGGL(swd_project_kernel<3>, dim3(grid), dim3(SWD_THREADS), lds, ctx->stream, plan, n, n_seg, d0, nd, width, x, off, mom, dirs, proj);
    RC_LAUNCH_CHECK(ctx);
  }
  return RCGAN_OK;
}

int rcgan_sort_rows_f32(rcgan_ctx* ctx, int rows, int width, float* x) {
  const bool ok = rows >= 1 && swd_pow2(width) && (long long)rows * width <= (1LL << 36) && x && ((uintptr_t)x & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "rows %d (>= 1), width %d (a power of two, rows * width <= 2^36), x %s", rows, width, x ? "given" : "NULL");
  if (width == 1) return RCGAN_OK;
  const int cw = width < SWD_SORT_CHUNK ? width : SWD_SORT_CHUNK;
  const size_t total = (size_t)rows * width;
  const unsigned chunks = (unsigned)(total / cw), pass_grid = (unsigned)((total / 2 + SWD_THREADS - 1) / SWD_THREADS);
  hipLaunchKernelGGL(swd_sort_local_kernel, dim3(chunks), dim3(SWD_THREADS), 0, ctx->stream, (uint32_t*)x, width, cw, 2, cw, 1);
  RC_LAUNCH_CHECK(ctx);
  for (long long k = 2LL * cw; k <= width; k <<= 1) {
    for (int j = (int)(k >> 1); j >= cw; j >>= 1) {
      hipLaunchKernelGGL(swd_sort_global_kernel, dim3(pass_grid), dim3(SWD_THREADS), 0, ctx->stream, (uint32_t*)x, total / 2, width, (int)k, j);
      RC_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(swd_sort_local_kernel, dim3(chunks), dim3(SWD_THREADS), 0, ctx->stream, (uint32_t*)x, width, cw, (int)k, (int)k, cw >> 1);
    RC_LAUNCH_CHECK(ctx);
  }
  return RCGAN_OK;
}

int rcgan_absdiff_rowsum(rcgan_ctx* ctx, int rows, int width, int n_seg, const int32_t* count, const float* a, const float* b, double* out) {
  const bool ok = rows >= 1 && width >= 1 && n_seg >= 1 && count && a && b && out && ((uintptr_t)count & 3) == 0 && ((uintptr_t)a & 3) == 0 &&
                  ((uintptr_t)b & 3) == 0 && ((uintptr_t)out & 7) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "rows %d, width %d, n_seg %d (>= 1 each), count / a / b / out %s", rows, width, n_seg, count && a && b && out ? "given" : "NULL");
  hipLaunchKernelGGL(swd_absdiff_rowsum_kernel, dim3(rows), dim3(SWD_THREADS), 0, ctx->stream, width, n_seg, count, a, b, out);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
