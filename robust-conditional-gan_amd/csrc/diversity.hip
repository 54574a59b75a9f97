// Diversity-sensitive generator term on same-label pairs (the definition is in include/rcgan_hip.h): for the pair of rows (i, i + P)
//   loss -= (weight / P) min(r_i, tau),  r_i = mean|x_i - x_{i+P}| / mean|z_i - z_{i+P}|,  and its gradient for x in the same launch.
// One workgroup per pair.  Both rows are read once: their differences stay in registers (16-byte route) or their signs in LDS
// (element-wise route) until the two block sums are known, and the gradient -+c sgn(difference) is written from them.  About 0.8 MB of
// traffic at P = 64, D = 3072 in 16-bit activations: the launch is bound by its latency, not by anything it computes.
#include <cmath>
#include "common.h"

namespace {

constexpr int DIV_BLOCK = 256;
constexpr int DIV_MAX_CHUNKS = 4;       // 16-byte chunks of one row per thread on the register route: rows of up to 1024 chunks
constexpr int DIV_LDS_MAX = 61440;      // element-wise route: one sign byte per element of a row

// 16 bytes of T, as floats
template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Chunk<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = bf16_to_f32((bf16_t)(w[j] & 0xffffu));
      v[2 * j + 1] = bf16_to_f32((bf16_t)(w[j] >> 16));
    }
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)f32_to_bf16(v[2 * j]) | ((uint32_t)f32_to_bf16(v[2 * j + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

struct DivArgs {
  int pairs, d, zdim;
  const void* x; const void* z; const int32_t* labels;
  float weight, tau;
  float* loss_acc; void* dx; int accumulate; float* ratio_out;
  float* part; unsigned* counter;         // the per-pair loss terms and their arrival counter (loss_acc != NULL)
  float gs_host; const float* gs_dev;
};

__device__ __forceinline__ float grad_scale_of(float gs_host, const float* gs_dev) { return gs_dev ? gs_host * gs_dev[0] : gs_host; }

// -c sgn(v): what row i of the pair gets; row i + P gets the negative
__device__ __forceinline__ float signed_step(float v, float c) { return v > 0.f ? -c : (v < 0.f ? c : 0.f); }

template <typename T, bool VEC>
__global__ __launch_bounds__(DIV_BLOCK) void pair_diversity_kernel(DivArgs a) {
  extern __shared__ __attribute__((aligned(16))) signed char sgn_lds[];   // element-wise route: the signs of the row's differences
  __shared__ float red[4];
  constexpr int N = Chunk<T>::N;
  const int i = blockIdx.x, tid = threadIdx.x;
  const size_t half = (size_t)a.pairs * a.d;
  const T* xa = (const T*)a.x + (size_t)i * a.d;
  const T* xb = xa + half;
  const T* za = (const T*)a.z + (size_t)i * a.zdim;
  const T* zb = za + (size_t)a.pairs * a.zdim;
  const bool same = a.labels == nullptr || a.labels[i] == a.labels[i + a.pairs];

  // ---- the two sums: a thread's elements in index order, then the fixed tree of block_sum256 ----
  float sz = 0.f;
  for (int k = tid; k < a.zdim; k += DIV_BLOCK) sz += fabsf(Elem<T>::ld(za + k) - Elem<T>::ld(zb + k));
  const float dz = block_sum256(sz, red) / (float)a.zdim;

  float diff[VEC ? DIV_MAX_CHUNKS : 1][N];
  const int chunks = a.d / N;
  float sx = 0.f;
  if (VEC) {
#pragma unroll
    for (int c = 0; c < DIV_MAX_CHUNKS; ++c) {
      const int q = tid + c * DIV_BLOCK;
      if (q < chunks) {
        float va[N], vb[N];
        Chunk<T>::ld(xa + (size_t)q * N, va);
        Chunk<T>::ld(xb + (size_t)q * N, vb);
#pragma unroll
        for (int j = 0; j < N; ++j) {
          diff[c][j] = va[j] - vb[j];
          sx += fabsf(diff[c][j]);
        }
      }
    }
  } else {
    for (int k = tid; k < a.d; k += DIV_BLOCK) {
      const float v = Elem<T>::ld(xa + k) - Elem<T>::ld(xb + k);
      sx += fabsf(v);
      sgn_lds[k] = (signed char)((v > 0.f) - (v < 0.f));        // read back below by the thread that wrote it
    }
  }
  const float di = block_sum256(sx, red) / (float)a.d;

  const bool live = same && dz != 0.f;                 // (uniform from here on: every thread holds the same sums)
  const float r = di / dz;
  const bool push = live && r < a.tau;                 // below the clamp: the pair has a gradient
  if (tid == 0 && a.ratio_out) a.ratio_out[i] = live ? r : -1.f;

  // ---- the gradient, from the values on chip ----
  if (a.dx && (push || !a.accumulate)) {
    const float c = push ? (a.weight * grad_scale_of(a.gs_host, a.gs_dev)) / ((float)a.pairs * (float)a.d * dz) : 0.f;
    T* da = (T*)a.dx + (size_t)i * a.d;
    T* db = da + half;
    if (VEC) {
#pragma unroll
      for (int cc = 0; cc < DIV_MAX_CHUNKS; ++cc) {
        const int q = tid + cc * DIV_BLOCK;
        if (q < chunks) {
          float ga[N], gb[N];
#pragma unroll
          for (int j = 0; j < N; ++j) {
            ga[j] = push ? signed_step(diff[cc][j], c) : 0.f;
            gb[j] = -ga[j];
          }
          if (a.accumulate) {
            float oa[N], ob[N];
            Chunk<T>::ld(da + (size_t)q * N, oa);
            Chunk<T>::ld(db + (size_t)q * N, ob);
#pragma unroll
            for (int j = 0; j < N; ++j) { ga[j] += oa[j]; gb[j] += ob[j]; }
          }
          Chunk<T>::st(da + (size_t)q * N, ga);
          Chunk<T>::st(db + (size_t)q * N, gb);
        }
      }
    } else {
      for (int k = tid; k < a.d; k += DIV_BLOCK) {
        float ga = push ? signed_step((float)sgn_lds[k], c) : 0.f, gb = -ga;
        if (a.accumulate) { ga += Elem<T>::ld(da + k); gb += Elem<T>::ld(db + k); }
        Elem<T>::st(da + k, ga);
        Elem<T>::st(db + k, gb);
      }
    }
  }

  // ---- the loss: one term per pair, summed in pair order by the last workgroup to arrive (as loss.hip's head does) ----
  if (tid == 0 && a.loss_acc) {
    const float term = live ? (r >= a.tau ? a.tau : r) : 0.f;
    __hip_atomic_store(a.part + i, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1u) {
      float tot = 0.f;
      for (unsigned w = 0; w < gridDim.x; ++w) tot += __hip_atomic_load(a.part + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *a.loss_acc += -(a.weight / (float)a.pairs) * tot;
      __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

extern "C" {

size_t rcgan_pair_diversity_workspace_bytes(int pairs) { return pairs > 0 ? (size_t)pairs * sizeof(float) : 0; }

int rcgan_pair_diversity_fwd_bwd(rcgan_ctx* ctx, int pairs, int d, int zdim, int dtype, const void* x, const void* z, const int32_t* labels,
                                 float weight, float tau, float* loss_acc, void* dx, int accumulate, float* ratio_out, void* ws,
                                 size_t ws_bytes) {
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  RC_REQUIRE(ctx, pairs >= 1 && d >= 1 && zdim >= 1, "%d pairs of rows of %d, latents of %d: at least one of each", pairs, d, zdim);
  RC_REQUIRE(ctx, x && z, "null pointer");
  const uintptr_t esz = dtype_size(dtype);
  RC_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)z | (uintptr_t)dx) & (esz - 1)) == 0, "x, z and dx must be aligned to their element (%d bytes)", (int)esz);
  RC_REQUIRE(ctx, (((uintptr_t)labels | (uintptr_t)loss_acc | (uintptr_t)ratio_out | (uintptr_t)ws) & 3) == 0,
             "labels, loss_acc, ratio_out and ws must be 4-byte aligned");
  RC_REQUIRE(ctx, std::isfinite(weight) && weight >= 0.f, "weight %g: finite and >= 0", (double)weight);
  RC_REQUIRE(ctx, tau > 0.f, "tau %g: > 0 (+inf: no clamp)", (double)tau);       // (false for a NaN too)
  if (weight == 0.f) return RCGAN_OK;
  const size_t row_bytes = (size_t)d * esz;
  const bool vec = row_bytes % 16 == 0 && row_bytes / 16 <= (size_t)DIV_MAX_CHUNKS * DIV_BLOCK && (((uintptr_t)x | (uintptr_t)dx) & 15) == 0;
  if (!vec && d > DIV_LDS_MAX)
    RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "rows of %d elements on the element-wise route (at most %d)", d, DIV_LDS_MAX);
  if (loss_acc) {
    const size_t need = rcgan_pair_diversity_workspace_bytes(pairs);
    if (!ws || ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
  }
  DivArgs a;
  a.pairs = pairs; a.d = d; a.zdim = zdim;
  a.x = x; a.z = z; a.labels = labels;
  a.weight = weight; a.tau = tau;
  a.loss_acc = loss_acc; a.dx = dx; a.accumulate = accumulate; a.ratio_out = ratio_out;
  a.part = (float*)ws; a.counter = ctx->counters() + RC_COUNTER_DIVERSITY;
  a.gs_host = ctx->gscale_host; a.gs_dev = ctx->gscale_dev;
  const size_t lds = vec ? 0 : (((size_t)d + 15) & ~(size_t)15);
  if (vec)
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL((pair_diversity_kernel<T, true>), dim3(pairs), dim3(DIV_BLOCK), 0, ctx->stream, a));
  else
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL((pair_diversity_kernel<T, false>), dim3(pairs), dim3(DIV_BLOCK), lds, ctx->stream, a));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
