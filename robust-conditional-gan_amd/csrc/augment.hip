// DiffAugment (Zhao et al., NeurIPS 2020) on the critic's input: colour jitter, integer translation and cutout of NHWC images
// [n, h, w, 3] as one launch, and its adjoint as one launch (rcgan_diffaugment_fwd / _bwd; the definition is in include/rcgan_hip.h).
//
// Both kernels are pure functions of (images, u, policy): the caller draws the eight uniforms of a sample.  One workgroup carries one
// sample: the sample is staged into LDS as fp32 with flat 4-element vector loads (the 3-channel interleave makes a pixel 12 bytes,
// so a pixel-per-thread walk over GLOBAL memory would be 12-byte strided), the per-pixel work then walks LDS one pixel per thread --
// three dword reads at a stride of 3 dwords between lanes, which is conflict-free on 32 banks -- into a second LDS image, and that
// image leaves with flat 4-element vector stores.  The two per-sample means are sums over a fixed assignment of pixels to threads,
// finished by block_sum256 (butterfly inside a wavefront, the four wavefronts in order): no atomics, the same bits every run.
// (The flat loops carry "vectorize(disable)": left to itself the loop vectoriser interleaves eight iterations and takes the 16-byte
// accesses apart into dword ones.)
//
// The adaptive probability (Karras et al., NeurIPS 2020) on top: rcgan_diffaugment_gated_fwd / rcgan_diffaugment_sampled_bwd are the
// same two bodies with the policy as a per-workgroup value -- the launch's policy masked by gate_u[b][t] < *p_dev, p read on the
// device when the launch runs, the result recorded per sample for the adjoint -- and rcgan_ada_update is the one-workgroup controller
// that moves p by the sign of E[sign D(real)] - target.
#include "common.h"

namespace {

constexpr int AUG_BLOCK = 256;
// dynamic LDS of a launch: the sample and its transform, 2 h w 3 floats.  Up to 64 KiB needs nothing; beyond that the kernel's limit is
// raised once per kernel (aug_lds_limit) to what a workgroup can have on gfx950 beside the four floats of the reduction.
constexpr size_t AUG_LDS_DEFAULT = 64 * 1024;
constexpr size_t AUG_LDS_MAX = 160 * 1024 - 256;

struct AugParams {
  float b, s, k;      // brightness offset, saturation factor, contrast factor
  int ty, tx;         // translation: out[p][q] = in[p + ty][q + tx]
  int r0, r1, c0, c1; // cutout window, inclusive (empty when r0 > r1)
};

__device__ __forceinline__ int aug_index(float u, int count) {   // min(floor(u * count), count - 1)
  const int i = (int)floorf(u * (float)count);
  return i < count - 1 ? i : count - 1;
}

__device__ __forceinline__ AugParams aug_params(const float* __restrict__ u, int h, int w, int policy) {
  AugParams p;
  p.b = u[0] - 0.5f;
  p.s = 2.f * u[1];
  p.k = u[2] + 0.5f;
  p.ty = p.tx = 0;
  if (policy & RCGAN_AUG_TRANSLATION) {
    const int sh = (h + 4) / 8, sw = (w + 4) / 8;
    p.ty = aug_index(u[3], 2 * sh + 1) - sh;
    p.tx = aug_index(u[4], 2 * sw + 1) - sw;
  }
  p.r0 = p.c0 = 1;
  p.r1 = p.c1 = 0;
  if (policy & RCGAN_AUG_CUTOUT) {
    const int oy = aug_index(u[5], h + 1), ox = aug_index(u[6], w + 1);
    p.r0 = max(oy - h / 4, 0);
    p.r1 = min(oy + h / 4 - 1, h - 1);
    p.c0 = max(ox - w / 4, 0);
    p.c1 = min(ox + w / 4 - 1, w - 1);
  }
  return p;
}

__device__ __forceinline__ bool aug_cut(const AugParams& p, int r, int c) { return r >= p.r0 && r <= p.r1 && c >= p.c0 && c <= p.c1; }

// four consecutive elements as one access: 16 bytes of fp32, 8 bytes of the 16-bit format
__device__ __forceinline__ float4 aug_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 aug_ld4(const bf16_t* p) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  return make_float4(bf16_to_f32((bf16_t)(t.x & 0xffffu)), bf16_to_f32((bf16_t)(t.x >> 16)),
                     bf16_to_f32((bf16_t)(t.y & 0xffffu)), bf16_to_f32((bf16_t)(t.y >> 16)));
}
__device__ __forceinline__ void aug_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void aug_st4(bf16_t* p, float4 v) {
  uint2 t;
  t.x = (uint32_t)f32_to_bf16(v.x) | ((uint32_t)f32_to_bf16(v.y) << 16);
  t.y = (uint32_t)f32_to_bf16(v.z) | ((uint32_t)f32_to_bf16(v.w) << 16);
  *reinterpret_cast<uint2*>(p) = t;
}
// the value a store to T leaves behind
template <typename T> __device__ __forceinline__ float aug_round(float v);
template <> __device__ __forceinline__ float aug_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float aug_round<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// y[b] = A_u(x[b]); y_pool[b] = the 2x2 mean of the STORED y[b], summed as meanpool2_fwd_kernel sums it.  The body of both forward
// kernels: `policy` is a per-workgroup value (the launch's, or the sample's own in the gated form).
template <typename T>
__device__ __forceinline__ void diffaugment_fwd_body(float4* aug_lds, float* red, int h, int w, int policy, const T* __restrict__ x,
                                                     const float* __restrict__ u, T* __restrict__ y, T* __restrict__ y_pool) {
  const int hw = h * w, cnt = hw * 3, tid = threadIdx.x;
  float* A = reinterpret_cast<float*>(aug_lds);      // the sample (after brightness and saturation); later the pooled output
  float* B = A + cnt;                                // the transformed sample as stored (cnt % 48 == 0: 16-byte aligned)
  const AugParams p = aug_params(u + 8 * (size_t)blockIdx.x, h, w, policy);
  const bool color = policy & RCGAN_AUG_COLOR;
  x += (size_t)blockIdx.x * cnt;
  y += (size_t)blockIdx.x * cnt;

  const float b = color ? p.b : 0.f;
#pragma clang loop vectorize(disable) interleave(disable)
  for (int v = tid; v < cnt / 4; v += AUG_BLOCK) {
    float4 t = aug_ld4(x + 4 * v);
    if (color) { t.x += b; t.y += b; t.z += b; t.w += b; }
    aug_lds[v] = t;
  }
  __syncthreads();

  float M = 0.f;
  if (color) {
    float part = 0.f;
    for (int px = tid; px < hw; px += AUG_BLOCK) {
      float* q = A + 3 * px;
      float a0 = q[0], a1 = q[1], a2 = q[2];
      const float m = ((a0 + a1) + a2) * (1.f / 3.f);
      a0 = fmaf(a0 - m, p.s, m);
      a1 = fmaf(a1 - m, p.s, m);
      a2 = fmaf(a2 - m, p.s, m);
      q[0] = a0; q[1] = a1; q[2] = a2;
      part += (a0 + a1) + a2;
    }
    M = block_sum256(part, red) * (1.f / (float)cnt);      // (its barriers also publish the writes above)
  }

  for (int px = tid; px < hw; px += AUG_BLOCK) {
    const int r = px / w, c = px - r * w;
    const int sr = r + p.ty, sc = c + p.tx;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (sr >= 0 && sr < h && sc >= 0 && sc < w && !aug_cut(p, r, c)) {
      const float* q = A + 3 * (sr * w + sc);
      v0 = q[0]; v1 = q[1]; v2 = q[2];
      if (color) {
        v0 = fmaf(v0 - M, p.k, M);
        v1 = fmaf(v1 - M, p.k, M);
        v2 = fmaf(v2 - M, p.k, M);
      }
    }
    float* o = B + 3 * px;
    o[0] = aug_round<T>(v0); o[1] = aug_round<T>(v1); o[2] = aug_round<T>(v2);
  }
  __syncthreads();

  const float4* B4 = reinterpret_cast<const float4*>(B);
#pragma clang loop vectorize(disable) interleave(disable)
  for (int v = tid; v < cnt / 4; v += AUG_BLOCK) aug_st4(y + 4 * v, B4[v]);
  if (y_pool == nullptr) return;

  const int ow = w / 2, row = 3 * w;
  for (int pp = tid; pp < hw / 4; pp += AUG_BLOCK) {
    const int r = pp / ow, c = pp - r * ow;
    const float* s = B + 3 * (2 * r * w + 2 * c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)       // add_n order of meanpool2_fwd_kernel: (0,0) + (1,0) + (0,1) + (1,1)
      A[3 * pp + ch] = aug_round<T>((((s[ch] + s[row + ch]) + s[3 + ch]) + s[row + 3 + ch]) * 0.25f);
  }
  __syncthreads();
  y_pool += (size_t)blockIdx.x * (cnt / 4);
#pragma clang loop vectorize(disable) interleave(disable)
  for (int v = tid; v < cnt / 16; v += AUG_BLOCK) aug_st4(y_pool + 4 * v, aug_lds[v]);
}

template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void diffaugment_fwd_kernel(int h, int w, int policy, const T* __restrict__ x,
                                                                     const float* __restrict__ u, T* __restrict__ y, T* __restrict__ y_pool) {
  extern __shared__ float4 aug_lds[];
  __shared__ float red[4];
  diffaugment_fwd_body<T>(aug_lds, red, h, w, policy, x, u, y, y_pool);
}

// the gated form: the sample's policy is the launch's, masked by gate_u[b][t] < *p_dev (p read HERE, on the device, when the launch
// runs), and is recorded for the adjoint.  !(g < p) is false for a NaN p: nothing is applied.
template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void diffaugment_gated_fwd_kernel(int h, int w, int policy, const T* __restrict__ x,
                                                                           const float* __restrict__ u, const float* __restrict__ gate_u,
                                                                           const float* __restrict__ p_dev, T* __restrict__ y,
                                                                           T* __restrict__ y_pool, int* __restrict__ sample_policy) {
  extern __shared__ float4 aug_lds[];
  __shared__ float red[4];
  const float p = *p_dev;
  const float* g = gate_u + 4 * (size_t)blockIdx.x;
  int mask = 0;
  if (g[0] < p) mask |= RCGAN_AUG_COLOR;
  if (g[1] < p) mask |= RCGAN_AUG_TRANSLATION;
  if (g[2] < p) mask |= RCGAN_AUG_CUTOUT;
  const int mine = __builtin_amdgcn_readfirstlane(policy & mask);      // the same in every lane: keep the branches on it scalar
  if (threadIdx.x == 0) sample_policy[blockIdx.x] = mine;
  diffaugment_fwd_body<T>(aug_lds, red, h, w, mine, x, u, y, y_pool);
}

// dx[b] (=|+=) A_u^T dy[b]: mask, shift back, then the adjoints of contrast and saturation (brightness adds a constant: no term).
// The body of both backward kernels, `policy` per workgroup as above.
template <typename T>
__device__ __forceinline__ void diffaugment_bwd_body(float4* aug_lds, float* red, int h, int w, int policy, const T* __restrict__ dy,
                                                     const float* __restrict__ u, T* __restrict__ dx, int accumulate) {
  const int hw = h * w, cnt = hw * 3, tid = threadIdx.x;
  float* A = reinterpret_cast<float*>(aug_lds);      // dy
  float* B = A + cnt;                                // the gradient at the input's pixels
  const AugParams p = aug_params(u + 8 * (size_t)blockIdx.x, h, w, policy);
  const bool color = policy & RCGAN_AUG_COLOR;
  dy += (size_t)blockIdx.x * cnt;
  dx += (size_t)blockIdx.x * cnt;

#pragma clang loop vectorize(disable) interleave(disable)
  for (int v = tid; v < cnt / 4; v += AUG_BLOCK) aug_lds[v] = aug_ld4(dy + 4 * v);
  __syncthreads();

  // g3: input pixel (r, c) was read by output pixel (r - ty, c - tx), if that one exists and is not cut out
  float part = 0.f;
  for (int px = tid; px < hw; px += AUG_BLOCK) {
    const int r = px / w, c = px - r * w;
    const int orow = r - p.ty, ocol = c - p.tx;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (orow >= 0 && orow < h && ocol >= 0 && ocol < w && !aug_cut(p, orow, ocol)) {
      const float* q = A + 3 * (orow * w + ocol);
      g0 = q[0]; g1 = q[1]; g2 = q[2];
    }
    float* o = B + 3 * px;
    o[0] = g0; o[1] = g1; o[2] = g2;
    part += (g0 + g1) + g2;
  }
  if (color) {
    const float mean = block_sum256(part, red) * (1.f / (float)cnt);
    const float km = (1.f - p.k) * mean, sm = 1.f - p.s;
    for (int px = tid; px < hw; px += AUG_BLOCK) {       // (a thread's own pixels: written above by itself)
      float* o = B + 3 * px;
      const float g0 = fmaf(p.k, o[0], km), g1 = fmaf(p.k, o[1], km), g2 = fmaf(p.k, o[2], km);
      const float mc = sm * (((g0 + g1) + g2) * (1.f / 3.f));
      o[0] = fmaf(p.s, g0, mc); o[1] = fmaf(p.s, g1, mc); o[2] = fmaf(p.s, g2, mc);
    }
  }
  __syncthreads();

  const float4* B4 = reinterpret_cast<const float4*>(B);
#pragma clang loop vectorize(disable) interleave(disable)
  for (int v = tid; v < cnt / 4; v += AUG_BLOCK) {
    float4 t = B4[v];
    if (accumulate) {
      const float4 o = aug_ld4(dx + 4 * v);
      t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
    }
    aug_st4(dx + 4 * v, t);
  }
}

template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void diffaugment_bwd_kernel(int h, int w, int policy, const T* __restrict__ dy,
                                                                     const float* __restrict__ u, T* __restrict__ dx, int accumulate) {
  extern __shared__ float4 aug_lds[];
  __shared__ float red[4];
  diffaugment_bwd_body<T>(aug_lds, red, h, w, policy, dy, u, dx, accumulate);
}

// the adjoint under the policy the gated forward recorded for the sample
template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void diffaugment_sampled_bwd_kernel(int h, int w, const T* __restrict__ dy, const float* __restrict__ u,
                                                                             const int* __restrict__ sample_policy, T* __restrict__ dx,
                                                                             int accumulate) {
  extern __shared__ float4 aug_lds[];
  __shared__ float red[4];
  const int all = RCGAN_AUG_COLOR | RCGAN_AUG_TRANSLATION | RCGAN_AUG_CUTOUT;
  const int mine = __builtin_amdgcn_readfirstlane(sample_policy[blockIdx.x] & all);
  diffaugment_bwd_body<T>(aug_lds, red, h, w, mine, dy, u, dx, accumulate);
}

// The controller of the augmentation probability (the definition is in include/rcgan_hip.h).  One workgroup: a strided loop over the
// rows, the signs summed by block_sum256 (a sum of small integers: exact in any order), the state written by thread 0.
__global__ __launch_bounds__(AUG_BLOCK) void ada_update_kernel(int n, const float* __restrict__ logits, int ld, const int* __restrict__ labels,
                                                                float* __restrict__ st, float target, float images, float interval) {
  __shared__ float red[4];
  float part = 0.f;
  for (int i = threadIdx.x; i < n; i += AUG_BLOCK) {
    const int c = labels ? labels[i] : 0;
    if (c < 0 || c >= ld) continue;                      // a label outside the row: the row counts as zero
    const float s = logits[(size_t)i * ld + c];
    part += (float)((s > 0.f) - (s < 0.f));
  }
  const float sum = block_sum256(part, red);
  if (threadIdx.x != 0) return;
  float p = st[0], sign_sum = st[1] + sum, count = st[2] + (float)n, steps = st[3] + 1.f;
  if (steps == interval) {
    const float r = sign_sum / count, d = r - target;
    p += (float)((d > 0.f) - (d < 0.f)) * count / images;
    p = fminf(fmaxf(p, 0.f), 1.f);
    st[0] = p;
    st[4] = r;
    st[5] += 1.f;
    sign_sum = count = steps = 0.f;
  }
  st[1] = sign_sum;
  st[2] = count;
  st[3] = steps;
}

// the argument checks of both entry points; -> LDS bytes of a launch
int aug_check(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* a, const void* u, const void* b, const void* pool, size_t* lds) {
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  RC_REQUIRE(ctx, n >= 1, "n = %d: at least one image", n);
  RC_REQUIRE(ctx, h >= 4 && w >= 4 && h % 4 == 0 && w % 4 == 0, "image size %d x %d: height and width must be multiples of 4", h, w);
  RC_REQUIRE(ctx, policy >= 0 && policy <= (RCGAN_AUG_COLOR | RCGAN_AUG_TRANSLATION | RCGAN_AUG_CUTOUT), "policy %d: a mask of COLOR = 1, TRANSLATION = 2, CUTOUT = 4", policy);
  RC_REQUIRE(ctx, a && u && b, "null pointer");
  *lds = (size_t)2 * h * w * 3 * sizeof(float);
  RC_REQUIRE(ctx, *lds <= AUG_LDS_MAX, "image size %d x %d x 3: the sample and its transform (%zu bytes of fp32) do not fit in %zu bytes of LDS",
             h, w, *lds, AUG_LDS_MAX);
  // the flat accesses move four elements: 16 bytes of fp32, 8 of the 16-bit format (a sample and its pooled output are whole vectors)
  const uintptr_t vec = 4 * dtype_size(dtype);
  RC_REQUIRE(ctx, (((uintptr_t)a | (uintptr_t)b | (uintptr_t)pool) & (vec - 1)) == 0 && ((uintptr_t)u & 3) == 0,
             "image pointers must be aligned to four elements (%d bytes)", (int)vec);
  return RCGAN_OK;
}

// a launch with more than the default 64 KiB of dynamic LDS: raise the kernel's limit to AUG_LDS_MAX, once
template <typename K>
int aug_lds_limit(rcgan_ctx* ctx, K kernel, size_t lds, bool* raised) {
  if (lds <= AUG_LDS_DEFAULT || *raised) return RCGAN_OK;
  RC_HIP(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AUG_LDS_MAX));
  *raised = true;
  return RCGAN_OK;
}

}  // namespace

extern "C" {

int rcgan_diffaugment_fwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* x, const float* u, void* y, void* y_pool) {
  size_t lds = 0;
  if (int rc = aug_check(ctx, n, h, w, dtype, policy, x, u, y, y_pool, &lds)) return rc;
  RC_DISPATCH_DTYPE(ctx, dtype, static bool raised = false; if (int rc = aug_lds_limit(ctx, diffaugment_fwd_kernel<T>, lds, &raised)) return rc;
                    hipLaunchKernelGGL(diffaugment_fwd_kernel<T>, dim3(n), dim3(AUG_BLOCK), lds, ctx->stream, h, w, policy,
                                                   (const T*)x, u, (T*)y, (T*)y_pool));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_diffaugment_bwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* dy, const float* u, void* dx, int accumulate) {
  size_t lds = 0;
  if (int rc = aug_check(ctx, n, h, w, dtype, policy, dy, u, dx, nullptr, &lds)) return rc;
  RC_DISPATCH_DTYPE(ctx, dtype, static bool raised = false; if (int rc = aug_lds_limit(ctx, diffaugment_bwd_kernel<T>, lds, &raised)) return rc;
                    hipLaunchKernelGGL(diffaugment_bwd_kernel<T>, dim3(n), dim3(AUG_BLOCK), lds, ctx->stream, h, w, policy,
                                                   (const T*)dy, u, (T*)dx, accumulate));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_diffaugment_gated_fwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* x, const float* u,
                                const float* gate_u, const float* p_dev, void* y, void* y_pool, int32_t* sample_policy) {
  size_t lds = 0;
  if (int rc = aug_check(ctx, n, h, w, dtype, policy, x, u, y, y_pool, &lds)) return rc;
  RC_REQUIRE(ctx, gate_u && p_dev && sample_policy, "null pointer");
  RC_REQUIRE(ctx, (((uintptr_t)gate_u | (uintptr_t)p_dev | (uintptr_t)sample_policy) & 3) == 0, "gate_u, p_dev and sample_policy must be 4-byte aligned");
  RC_DISPATCH_DTYPE(ctx, dtype, static bool raised = false; if (int rc = aug_lds_limit(ctx, diffaugment_gated_fwd_kernel<T>, lds, &raised)) return rc;
                    hipLaunchKernelGGL(diffaugment_gated_fwd_kernel<T>, dim3(n), dim3(AUG_BLOCK), lds, ctx->stream, h, w, policy,
                                                   (const T*)x, u, gate_u, p_dev, (T*)y, (T*)y_pool, (int*)sample_policy));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_diffaugment_sampled_bwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, const void* dy, const float* u,
                                  const int32_t* sample_policy, void* dx, int accumulate) {
  size_t lds = 0;
  if (int rc = aug_check(ctx, n, h, w, dtype, 0, dy, u, dx, nullptr, &lds)) return rc;
  RC_REQUIRE(ctx, sample_policy, "null pointer");
  RC_REQUIRE(ctx, ((uintptr_t)sample_policy & 3) == 0, "sample_policy must be 4-byte aligned");
  RC_DISPATCH_DTYPE(ctx, dtype, static bool raised = false; if (int rc = aug_lds_limit(ctx, diffaugment_sampled_bwd_kernel<T>, lds, &raised)) return rc;
                    hipLaunchKernelGGL(diffaugment_sampled_bwd_kernel<T>, dim3(n), dim3(AUG_BLOCK), lds, ctx->stream, h, w,
                                                   (const T*)dy, u, (const int*)sample_policy, (T*)dx, accumulate));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_ada_update(rcgan_ctx* ctx, int n, const float* logits, int ld, const int32_t* labels, float* ada_state, float target,
                     float images, int interval) {
  RC_REQUIRE(ctx, n >= 1 && ld >= 1, "n = %d rows of %d logits: at least one of each", n, ld);
  RC_REQUIRE(ctx, interval >= 1, "interval %d: at least one call per update", interval);
  RC_REQUIRE(ctx, images > 0.f, "images %g: the adjustment speed must be positive", (double)images);
  RC_REQUIRE(ctx, logits && ada_state, "null pointer");
  RC_REQUIRE(ctx, (((uintptr_t)logits | (uintptr_t)ada_state | (uintptr_t)labels) & 3) == 0, "logits, labels and ada_state must be 4-byte aligned");
  hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(AUG_BLOCK), 0, ctx->stream, n, logits, ld, (const int*)labels, ada_state, target, images,
                     (float)interval);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
