// Azimuthally averaged power spectrum of small square images (spectrum.py: the radial power-spectrum distance).  Definition (restated
// in float64 by tests/spectrum_ref.py): images uint8 NHWC x[n][N][N][c], c 1 or 3, 8 <= N <= 32;
//   a = x - 128 (exact),  F_ch(u,v) = sum_{y,x} a[y][x][ch] exp(-2 pi i (u y + v x) / N),  P = |F|^2 / N^2;
//   f(u) = u if u <= N / 2 (integer division) else u - N;  the ring of (u,v) is the integer b with
//   (2b - 1)^2 <= 4 (f(u)^2 + f(v)^2) < (2b + 1)^2, ring 0 the point (0,0) alone -- integer arithmetic, no square root;
//   B(N) = 1 + the ring of (N/2, N/2) (24 at 32, 21 at 28, 7 at 9);  out[i][ch][b] = the mean of P over the members of ring b.
//
// spectrum_kernel (rcgan_radial_spectrum): one workgroup of 256 threads walks images blockIdx.x, blockIdx.x + gridDim.x, ...  It keeps
// in LDS the twiddle tables C[x][v] = cos(2 pi ((x v) mod N) / N) and S likewise (both symmetric), the centred image as fp32 planes
// A[ch][y][x], one channel's first-pass results Yc = A C and Ys = A S, that channel's |F|^2 in fp64 and the ring of every (u,v); every
// plane is 32 x 32 and starts as zeros, and nothing is ever written at an index >= N, so a smaller N is its own transform and not a
// padded one.  The 2 x 32 cosines and sines of 2 pi k / N are computed in float64 on the host and travel as fp32 kernel arguments (256
// bytes): no upload, no device sinf / cosf, nothing for a captured graph to depend on.
// Per channel, with W = C - i S:  Re F = C Yc - S Ys,  Im F = -(C Ys + S Yc): six N x N x N real products on the vector units.  Thread t
// owns column v = t % 32 and rows t / 32 + {0, 8, 16, 24}: in pass one a lane reads C[x][v], S[x][v] (consecutive banks) and four
// broadcast A[y][x] for eight fused multiply-adds; in pass two Yc[y][v], Ys[y][v] and eight broadcast twiddles for sixteen.  (The
// fp32 matrix cores, v_mfma_f32_32x32x2_f32, would take the same products; at 6 10^9 multiply-adds for 10 000 images the vector form
// is already far below the cost of moving the images to the device: DESIGN section 3.)
// Ring sums: thread t scans (u,v) = t % 8, t % 8 + 8, ... in index order for ring t / 8 and adds the members in fp64; the eight
// partials of a ring are added in the order 0..7 by one thread, which divides by (members N^2) and rounds once to fp32.  The order is
// fixed by the launch geometry, there are no atomics: the same bits on every run, eager or replayed.
// LDS: 2 (twiddles) + c (image) + 2 (Yc, Ys) planes of 4 KiB, 8 KiB of |F|^2, 1 KiB of rings, 2.5 KiB of partials: 39.5 KiB at c = 3.
//
// Arithmetic and its bound (u = 2^-24).  a is an integer of at most 128 in magnitude, exact.  A twiddle is the fp32 rounding of a
// float64 value that is itself within 2^-52 of the truth: t^ = t (1 + e), |e| <= u (1 + 2^-27).  Pass one is a chain of N fused
// multiply-adds per entry (terms at an index >= N do not exist), pass two is four chains of N (C Yc, S Ys, C Ys, S Yc), then one
// subtraction or addition (the sign change is exact).  Following one term a[y][x] t1 t2 to its place in Re F^ or Im F^, it is
// multiplied by at most 2 (twiddles) + N (pass one) + N (pass two) + 1 (the last operation) = 2N + 3 factors (1 + e_k), |e_k| <= u
// (1 + 2^-27).  The constant used is 2N + 8, which leaves room for the 2^-27:
//     |Re F^ - Re F| <= gamma sum_{y,x} |a| (|cos cos| + |sin sin|) <= gamma sum |a|,   gamma = (2N + 8) u / (1 - (2N + 8) u),
// likewise Im (|cos sin| + |sin cos| <= 1), so
//     |F^ - F| <= delta = g sum_{y,x} |a[y][x][ch]|,     g = sqrt(2) gamma.
// |F^|^2 = (double)re^2 + (double)im^2 has exact products and one fp64 rounding; a ring's fp64 sum of m <= 94 such values, the
// division and the product with 1 / N^2 add at most (m + 3) 2^-53 relative, and | |F^|^2 - |F|^2 | <= 2 |F| delta + delta^2.  The
// result is rounded once to fp32 (u relative, or 2^-150 absolute below the normal range).  With E = (2 mean_ring|F| delta + delta^2)
// / N^2 and `exact` the true ring mean,
//     |out - exact| <= E + 2 u (exact + E) + 2^-149
// (tests/spectrum_ref.py: ``bound``; the test asserts exactly this).  An image of 128s has a = 0 and gives exact zeros.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)     // (the fused operations are the ones written as fmaf: the error analysis above counts them)

#define SP_THREADS 256
#define SP_LD 32                     // every plane is 32 x 32
#define SP_PLANE (SP_LD * SP_LD)
#define SP_MIN_N 8
#define SP_MAX_N 32

struct SpTwiddles {
  float c[SP_MAX_N], s[SP_MAX_N];    // cos / sin of 2 pi k / N, k < N; zeros behind
};

// the ring of the signed frequency pair (fu, fv): the b with (2b - 1)^2 <= 4 (fu^2 + fv^2) < (2b + 1)^2
__host__ __device__ static inline int sp_ring(int fu, int fv) {
  const int r2 = 4 * (fu * fu + fv * fv);
  int b = 0;
  while ((2 * b + 1) * (2 * b + 1) <= r2) ++b;
  return b;
}

static int sp_rings(int N) { return 1 + sp_ring(N / 2, N / 2); }

template <int CH>
__global__ __launch_bounds__(SP_THREADS) void spectrum_kernel(int n, int N, int B, int vec, SpTwiddles tw, const uint8_t* __restrict__ x,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tc[SP_PLANE], ts[SP_PLANE], img[CH * SP_PLANE], yc[SP_PLANE], ys[SP_PLANE];
  __shared__ double pw[SP_PLANE];                 // |F|^2 of the channel at hand, [u][v]
  __shared__ double part[SP_THREADS];             // ring partials, [ring][8]
  __shared__ int members[SP_LD];
  __shared__ uint8_t ring[SP_PLANE];              // [u][v], u, v < N
  const int tid = threadIdx.x, v = tid & 31, r0 = tid >> 5;
  const int half = N / 2, pixels = N * N * CH;

  for (int t = tid; t < SP_PLANE; t += SP_THREADS) {
    const int a = t >> 5, b = t & 31;
    const bool in = a < N && b < N;
    const int k = in ? (a * b) % N : 0;
    tc[t] = in ? tw.c[k] : 0.f;
    ts[t] = in ? tw.s[k] : 0.f;
    yc[t] = 0.f;
    ys[t] = 0.f;
    pw[t] = 0.0;
    ring[t] = in ? (uint8_t)sp_ring(a <= half ? a : a - N, b <= half ? b : b - N) : (uint8_t)255;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) img[ch * SP_PLANE + t] = 0.f;
  }
  __syncthreads();

  for (long i = blockIdx.x; i < n; i += gridDim.x) {
    const uint8_t* src = x + (size_t)i * pixels;
    if (vec) {                                    // (x 16-byte aligned and an image a multiple of 16 bytes)
      for (int q = tid; q < pixels / 16; q += SP_THREADS) {
        const uint4 w4 = ((const uint4*)src)[q];
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int e = q * 16 + j, ch = e % CH, p = e / CH;
          img[ch * SP_PLANE + (p / N) * SP_LD + p % N] = (float)((int)((w[j >> 2] >> (8 * (j & 3))) & 255u) - 128);
        }
      }
    } else {
      for (int e = tid; e < pixels; e += SP_THREADS) {
        const int ch = e % CH, p = e / CH;
        img[ch * SP_PLANE + (p / N) * SP_LD + p % N] = (float)((int)src[e] - 128);
      }
    }
    __syncthreads();

    for (int ch = 0; ch < CH; ++ch) {
      const float* A = img + ch * SP_PLANE;
      // pass one: Yc = A C, Ys = A S (rows r0 + 8 k, column v; rows and columns >= N come out as the zeros they hold already)
      if (v < N) {
        float ac[4] = {0.f, 0.f, 0.f, 0.f}, as[4] = {0.f, 0.f, 0.f, 0.f};
        for (int xx = 0; xx < N; ++xx) {
          const float c = tc[xx * SP_LD + v], s = ts[xx * SP_LD + v];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float a = A[(r0 + 8 * k) * SP_LD + xx];
            ac[k] = fmaf(a, c, ac[k]);
            as[k] = fmaf(a, s, as[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (r0 + 8 * k < N) {
            yc[(r0 + 8 * k) * SP_LD + v] = ac[k];
            ys[(r0 + 8 * k) * SP_LD + v] = as[k];
          }
        }
      }
      __syncthreads();
      // pass two: Re F = C Yc - S Ys, Im F = -(C Ys + S Yc)
      if (v < N) {
        float cc[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f}, cs[4] = {0.f, 0.f, 0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int y = 0; y < N; ++y) {
          const float pc = yc[y * SP_LD + v], ps = ys[y * SP_LD + v];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float c = tc[(r0 + 8 * k) * SP_LD + y], s = ts[(r0 + 8 * k) * SP_LD + y];
            cc[k] = fmaf(c, pc, cc[k]);
            ss[k] = fmaf(s, ps, ss[k]);
            cs[k] = fmaf(c, ps, cs[k]);
            sc[k] = fmaf(s, pc, sc[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (r0 + 8 * k < N) {
            const double re = (double)(cc[k] - ss[k]), im = (double)(-(cs[k] + sc[k]));
            pw[(r0 + 8 * k) * SP_LD + v] = re * re + im * im;
          }
        }
      }
      __syncthreads();
      // ring sums: ring tid / 8, the members among (u,v) = tid % 8, tid % 8 + 8, ... in index order
      {
        const int b = tid >> 3;
        double acc = 0.0;
        int cnt = 0;
        if (b < B) {
          for (int e = tid & 7; e < N * N; e += 8) {
            const int at = (e / N) * SP_LD + e % N;
            if (ring[at] == b) {
              acc += pw[at];
              ++cnt;
            }
          }
        }
        part[tid] = acc;
        // (a ring's member count: an integer, any order)
        for (int o = 4; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 8);
        if ((tid & 7) == 0) members[b] = cnt;
      }
      __syncthreads();
      if (tid < B) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += part[tid * 8 + j];
        out[((size_t)i * CH + ch) * B + tid] = (float)(s / ((double)members[tid] * (double)(N * N)));
      }
      // (the next channel's pass one writes yc / ys, which pass two has finished reading; its pass two writes pw after the barrier
      // that follows pass one, and part / members after two more: this channel's readers of them are past by then)
    }
    __syncthreads();                              // the next image overwrites img
  }
}

extern "C" {

int rcgan_radial_spectrum(rcgan_ctx* ctx, int n, int N, int c, const uint8_t* x, float* out) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool ok = n >= 1 && N >= SP_MIN_N && N <= SP_MAX_N && (c == 1 || c == 3) && x && out && ((uintptr_t)out & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d (>= 1), N %d (%d..%d), c %d (1 or 3), x / out (4-byte aligned) %s", n, N, SP_MIN_N, SP_MAX_N, c,
             x && out ? "given" : "NULL");
  SpTwiddles tw;
  const double step = 2.0 * 3.14159265358979323846 / (double)N;
  for (int k = 0; k < SP_MAX_N; ++k) {
    tw.c[k] = k < N ? (float)cos(step * (double)k) : 0.f;
    tw.s[k] = k < N ? (float)sin(step * (double)k) : 0.f;
  }
  const int B = sp_rings(N);
  const int vec = ((uintptr_t)x & 15) == 0 && (N * N * c) % 16 == 0 ? 1 : 0;
  const int grid = n < 4 * ctx->num_cus ? n : 4 * ctx->num_cus;
  if (c == 1)
    hipLaunchKernelGGL(spectrum_kernel<1>, dim3(grid), dim3(SP_THREADS), 0, ctx->stream, n, N, B, vec, tw, x, out);
  else
    hipLaunchKernelGGL(spectrum_kernel<3>, dim3(grid), dim3(SP_THREADS), 0, ctx->stream, n, N, B, vec, tw, x, out);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
