// Per-scale SSIM means of image pairs (msssim.py: intra-class MS-SSIM, the image-space diversity of a class): for every pair (i, j)
// of a list and each of five dyadic scales, the mean over positions and channels of the contrast-structure map v1 / v2 and of the full
// SSIM map, as the reference's _SSIMForMultiScale computes them for a batch of one (cifar10/common/msssim.py), max_val 255,
// k1 0.01, k2 0.03.  At a level of h_l x w_l pixels the window is s = min(11, h_l, w_l) taps of a Gaussian with sigma 1.5 s / 11
// (the 'fspecial' form: centres at k - (s - 1) / 2, normalised), 'valid' positions only; the next level is the 2 x 2 mean at stride 2
// anchored at (0, 0), the last row / column averaged with itself where the size is odd: h_{l+1} = ceil(h_l / 2).
//
// 16 <= h, w <= 32 (MS_MIN_HW: below it a level would be empty; MS_MAX_HW: the LDS plan below, 46.0 KiB at 32 x 32 x 3), c 1 or 3.
//
// One workgroup of 256 threads per pair; nothing but `out` is written.  Both images are read once (16-byte loads where an image is a
// multiple of 16 bytes and the tensor 16-byte aligned) into LDS as fp32 planes [image][channel], raw 0..255; the four coarser levels
// of every plane are built behind them (a pyramid of 1364 floats per plane at 32 x 32).  Then, level by level and channel by
// channel, a row pass writes five fields of h_l x (w_l - s + 1) floats and a column pass reads them, forms the two maps and keeps
// per-thread sums; per level the sums are merged by a butterfly inside each wavefront and the four wavefronts' sums are added in
// order -- no floating-point atomics, the order is fixed by the launch geometry: the same bits on every run.
// LDS: 320 B + 4 (2 c sum_l h_l w_l + 5 h (w - 10)) B: 46.0 KiB at 32 x 32 x 3 (three workgroups per CU), 18.4 KiB at 28 x 28 x 1.
//
// Arithmetic: fp32 throughout, and no subtraction of two large second moments.  With g the fp32-rounded taps (computed in float64 on
// the host; S = sum g, |S - 1| <= u, u = 2^-24), the row pass computes per row r and output column, over the s pixels a_k, b_k of the
// two images under the window,
//     m_a = sum_k g_k a_k   (a chain of s fused multiply-adds; likewise m_b)
//     q_aa = sum_k g_k (a_k - m_a)^2      q_bb likewise      q_ab = sum_k g_k (a_k - m_a)(b_k - m_b)
// and the column pass, over the s rows under the window,
//     mu_a = sum_r g_r m_a[r]             s_aa = sum_r g_r (q_aa[r] + (m_a[r] - mu_a)^2)      s_bb, s_ab likewise.
// By the law of total variance s_aa is S^2 (1 + O(u)) times the variance of the window under the weights g g / S^2, whatever the
// centres m and mu are as long as they are within ~1e-4 of the weighted means (they are: the error of a chain of s <= 11 fused
// multiply-adds on values in [0, 255]); those weights differ from the reference's float64 taps by a relative 4 u.  Every term of s_aa
// is non-negative, so its roundings are relative; what is absolute is the error e <= 11.1 u 255 = 1.7e-4 of a row mean m[r] against
// the exact weighted mean, which moves the spread of the row means by at most e: with sd_a = sqrt(sigma_aa)
//     |s_aa - sigma_aa| <= 64 u sigma_aa + 2 e sd_a + 1e-6        |s_ab - sigma_ab| <= 64 u sd_a sd_b + e (sd_a + sd_b) + 1e-6.
// (Pixels of level l are multiples of 4^-l below 256: exact in fp32, so is the pyramid.)  With v1 = 2 s_ab + c2, v2 = s_aa + s_bb + c2,
// c2 = (0.03 * 255)^2 = 58.5225, |v1 / v2| <= 1 and t = sd_a + sd_b, v2 >= t^2 / 2 + c2:
//     |cs_computed - cs| <= (64 u t^2 + 4 e t + 4e-6) / (t^2 / 2 + c2) + 8 u <= 128 u + 4 e / sqrt(2 c2) + 7e-8 + 8 u <= 7.2e-5
// at every position.  The means mu carry a RELATIVE error of at most 26 u (taps included), so the luminance factor
// (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1) <= 1 moves by at most 110 u = 6.6e-6, and a position's SSIM value by at most 8e-5.
// A mean over at most 22 * 22 * 3 positions (six per thread, a six-step butterfly, four partial sums) adds at most 20 u of the mean
// magnitude.  Hence, for every pair and scale,
//     |out - exact| <= 1e-4        (both the contrast-structure mean and the SSIM mean),
// with the same arithmetic and bound for identical images (exactly 1.0: a and b then take the same roundings) and constant images.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)     // (the fused operations are the ones written as fmaf: the error analysis above counts them)

#define MS_LEVELS 5
#define MS_WIN 11
#define MS_MIN_HW 16
#define MS_MAX_HW 32
#define MS_THREADS 256
#define MS_HEAD 80                   // floats in front of the planes: 55 taps (64 reserved), 8 wavefront partial sums (16 reserved)

struct MsPlan {
  int h[MS_LEVELS], w[MS_LEVELS], s[MS_LEVELS], off[MS_LEVELS];   // level size, window, offset (floats) of the level in a plane's pyramid
  int plane, field;                                               // floats per plane (all levels); floats per row-pass field
  float tap[MS_LEVELS * MS_WIN];
};

static void ms_plan(int h, int w, MsPlan* p) {
  int off = 0;
  p->field = 0;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int s = h < MS_WIN ? (h < w ? h : w) : (w < MS_WIN ? w : MS_WIN);
    p->h[l] = h; p->w[l] = w; p->s[l] = s; p->off[l] = off;
    off += h * w;
    if (h * (w - s + 1) > p->field) p->field = h * (w - s + 1);
    const double sigma = 1.5 * s / 11.0;
    double e[MS_WIN], sum = 0.0;
    for (int k = 0; k < s; ++k) {
      const double x = k - 0.5 * (s - 1);
      e[k] = exp(-(x * x) / (2.0 * sigma * sigma));
      sum += e[k];
    }
    for (int k = 0; k < MS_WIN; ++k) p->tap[l * MS_WIN + k] = k < s ? (float)(e[k] / sum) : 0.f;
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  p->plane = off;
}

static size_t ms_lds_bytes(const MsPlan& p, int c) { return sizeof(float) * ((size_t)MS_HEAD + 2 * (size_t)c * p.plane + 5 * (size_t)p.field); }

__global__ __launch_bounds__(MS_THREADS) void msssim_pairs_kernel(MsPlan P, int n, int c, int vec, const uint8_t* __restrict__ x,
                                                                  const int32_t* __restrict__ pairs, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ms_smem[];
  float* taps = ms_smem;
  float* red = ms_smem + 64;
  float* img = ms_smem + MS_HEAD;                        // [2][c][P.plane]
  float* fld = img + 2 * c * P.plane;                    // [5][P.field]: m_a, m_b, q_aa, q_bb, q_ab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = pairs[2 * (size_t)blockIdx.x], j = pairs[2 * (size_t)blockIdx.x + 1];
  float* o = out + 10 * (size_t)blockIdx.x;
  if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) {         // (the whole workgroup: no barrier has been met)
    if (tid < 10) o[tid] = __builtin_nanf("");
    return;
  }
  if (tid < MS_LEVELS * MS_WIN) taps[tid] = P.tap[tid];
  const int bytes = P.h[0] * P.w[0] * c;
  for (int im = 0; im < 2; ++im) {
    const uint8_t* src = x + (size_t)(im ? j : i) * bytes;
    float* dst = img + im * c * P.plane;
    if (vec) {
      for (int q = tid; q < bytes / 16; q += MS_THREADS) {
        const uint4 v = ((const uint4*)src)[q];
        const unsigned word[4] = {v.x, v.y, v.z, v.w};
        int pix = 16 * q / c, ch = 16 * q - pix * c;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          dst[ch * P.plane + pix] = (float)((word[b >> 2] >> (8 * (b & 3))) & 255u);
          if (++ch == c) { ch = 0; ++pix; }
        }
      }
    } else {
      for (int e = tid; e < bytes; e += MS_THREADS) {
        const int pix = e / c, ch = e - pix * c;
        dst[ch * P.plane + pix] = (float)src[e];
      }
    }
  }
  __syncthreads();
  // the pyramid: level l of every plane out of level l - 1 (sums of four multiples of 4^-(l-1) below 256: exact)
  for (int l = 1; l < MS_LEVELS; ++l) {
    const int hi = P.h[l - 1], wi = P.w[l - 1], ho = P.h[l], wo = P.w[l];
    for (int t = tid; t < 2 * c * ho * wo; t += MS_THREADS) {
      const int pl = t / (ho * wo), r = t - pl * ho * wo, y = r / wo, xx = r - y * wo;
      const float* s = img + pl * P.plane + P.off[l - 1];
      const int y0 = 2 * y, y1 = min(2 * y + 1, hi - 1), x0 = 2 * xx, x1 = min(2 * xx + 1, wi - 1);
      img[pl * P.plane + P.off[l] + r] = ((s[y0 * wi + x0] + s[y0 * wi + x1]) + (s[y1 * wi + x0] + s[y1 * wi + x1])) * 0.25f;
    }
    __syncthreads();
  }
  const float c1 = 6.5025f, c2 = 58.5225f;               // (0.01 * 255)^2, (0.03 * 255)^2
  const int F = P.field;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int hl = P.h[l], wl = P.w[l], s = P.s[l], wo = wl - s + 1, ho = hl - s + 1;
    const float* g = taps + l * MS_WIN;
    float sum_cs = 0.f, sum_ssim = 0.f;
    for (int ch = 0; ch < c; ++ch) {
      const float* A = img + ch * P.plane + P.off[l];
      const float* B = img + (c + ch) * P.plane + P.off[l];
      for (int t = tid; t < hl * wo; t += MS_THREADS) {                  // the row pass
        const int r = t / wo, col = t - r * wo;
        const float* a = A + r * wl + col;
        const float* b = B + r * wl + col;
        float ma = 0.f, mb = 0.f, qaa = 0.f, qbb = 0.f, qab = 0.f;
        for (int k = 0; k < s; ++k) {
          ma = fmaf(g[k], a[k], ma);
          mb = fmaf(g[k], b[k], mb);
        }
        for (int k = 0; k < s; ++k) {
          const float da = a[k] - ma, db = b[k] - mb, ta = g[k] * da, tb = g[k] * db;
          qaa = fmaf(ta, da, qaa);
          qbb = fmaf(tb, db, qbb);
          qab = fmaf(ta, db, qab);
        }
        fld[t] = ma; fld[F + t] = mb; fld[2 * F + t] = qaa; fld[3 * F + t] = qbb; fld[4 * F + t] = qab;
      }
      __syncthreads();
      for (int t = tid; t < ho * wo; t += MS_THREADS) {                  // the column pass and the two maps
        const float* f = fld + t;                                       // (row t / wo, column t % wo: the window's first row)
        float ua = 0.f, ub = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
        for (int r = 0; r < s; ++r) {
          ua = fmaf(g[r], f[r * wo], ua);
          ub = fmaf(g[r], f[F + r * wo], ub);
        }
        for (int r = 0; r < s; ++r) {
          const float da = f[r * wo] - ua, db = f[F + r * wo] - ub;
          saa = fmaf(g[r], f[2 * F + r * wo] + da * da, saa);
          sbb = fmaf(g[r], f[3 * F + r * wo] + db * db, sbb);
          sab = fmaf(g[r], f[4 * F + r * wo] + da * db, sab);
        }
        const float cs = (2.f * sab + c2) / (saa + sbb + c2);
        const float lum = (2.f * (ua * ub) + c1) / (ua * ua + ub * ub + c1);
        sum_cs += cs;
        sum_ssim += lum * cs;
      }
      __syncthreads();                                                   // (the next row pass overwrites the fields)
    }
    sum_cs = wave_sum(sum_cs);
    sum_ssim = wave_sum(sum_ssim);
    if (lane == 0) { red[wave] = sum_cs; red[4 + wave] = sum_ssim; }
    __syncthreads();
    if (tid == 0) {                                                      // (red is next written behind the next level's barriers)
      const float count = (float)(ho * wo * c);
      o[l] = ((red[0] + red[1]) + (red[2] + red[3])) / count;
      o[MS_LEVELS + l] = ((red[4] + red[5]) + (red[6] + red[7])) / count;
    }
  }
}

extern "C" {

int rcgan_msssim_pairs(rcgan_ctx* ctx, int n, int h, int w, int c, int n_pairs, const uint8_t* x, const int32_t* pairs, float* out) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool ok = n >= 1 && n_pairs >= 1 && (c == 1 || c == 3) && h >= MS_MIN_HW && h <= MS_MAX_HW && w >= MS_MIN_HW && w <= MS_MAX_HW &&
                  x && pairs && out && ((uintptr_t)pairs & 3) == 0 && ((uintptr_t)out & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d, n_pairs %d (>= 1), h %d, w %d (%d..%d), c %d (1 or 3), x / pairs / out %s", n, n_pairs, h, w, MS_MIN_HW, MS_MAX_HW, c,
             x && pairs && out ? "given" : "NULL");
  MsPlan plan;
  ms_plan(h, w, &plan);
  const int vec = (h * w * c) % 16 == 0 && ((uintptr_t)x & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(msssim_pairs_kernel, dim3(n_pairs), dim3(MS_THREADS), ms_lds_bytes(plan, c), ctx->stream, plan, n, c, vec, x, pairs, out);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
