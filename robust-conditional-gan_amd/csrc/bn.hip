// Batch norm / conditional batch norm (+ fused activation), forward and backward.
//   reference: tf.contrib.layers.batch_norm (mnist/ops.py:38-44) and
//   tf.nn.moments + embedding_lookup + tf.nn.batch_normalization (cifar10/common/ops/normalization.py:47-57).
// HBM-bound: x is read once for the statistics and once for the apply; the backward reads (x, y, dy)
// once for the per-group sums and once for the apply.  Reductions are two-level and deterministic
// (per-row-group partials in fp32, combined in fp64) -- no atomics.
#include "common.h"
#include "conv_mfma.h"
#include "bn_plan.h"

// partial[g][0][c] = sum_rows v1, partial[g][1][c] = sum_rows v2 over row group g (rows_per_group rows)
// MODE 0: (x, x*x)         MODE 1: (dy', dy'*xhat) with dy' = dy*act'(y), xhat = (x-mean)*rstd
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_partial_kernel(long rows, int c, long rows_per_group, const T* x, const T* y,
                                                         const T* dy, const float* mean, const float* rstd, int act,
                                                         float* partial) {
  __shared__ float red[2][4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const long rb = (long)blockIdx.y * rows_per_group;
  long re = rb + rows_per_group;
  if (re > rows) re = rows;
  float s1 = 0.f, s2 = 0.f;
  if (col < c) {
    float mu = 0.f, rs = 1.f;
    if (MODE == 1) { mu = mean[col]; rs = rstd[col]; }
    for (long r = rb + rl; r < re; r += 4) {
      const long off = r * c + col;
      if (MODE == 0) {
        float v = Elem<T>::ld(x + off);
        s1 += v; s2 += v * v;
      } else {
        float g = Elem<T>::ld(dy + off);
        if (act != RCGAN_ACT_NONE) g *= act_grad(act, Elem<T>::ld(y + off));
        float xh = (Elem<T>::ld(x + off) - mu) * rs;
        s1 += g; s2 += g * xh;
      }
    }
  }
  red[0][rl][threadIdx.x & 63] = s1;
  red[1][rl][threadIdx.x & 63] = s2;
  __syncthreads();
  if (threadIdx.x < 64 && col < c) {
    const int t = threadIdx.x;
    partial[((long)blockIdx.y * 2 + 0) * c + col] = red[0][0][t] + red[0][1][t] + red[0][2][t] + red[0][3][t];
    partial[((long)blockIdx.y * 2 + 1) * c + col] = red[1][0][t] + red[1][1][t] + red[1][2][t] + red[1][3][t];
  }
}

__global__ void bn_stats_finalize_kernel(int c, int ngroups, long rows, const float* partial, float eps, float* mean,
                                         float* rstd, float* mm, float* mv, float decay) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= c) return;
  double s1 = 0.0, s2 = 0.0;
  for (int g = 0; g < ngroups; ++g) {
    s1 += (double)partial[((long)g * 2 + 0) * c + col];
    s2 += (double)partial[((long)g * 2 + 1) * c + col];
  }
  double mu = s1 / (double)rows;
  double var = s2 / (double)rows - mu * mu;
  if (var < 0.0) var = 0.0;
  mean[col] = (float)mu;
  rstd[col] = (float)(1.0 / sqrt(var + (double)eps));
  if (mm) {
    // TF fused batch norm: moving -= (moving - batch) * (1 - decay), variance with Bessel's correction
    double uvar = rows > 1 ? var * ((double)rows / (double)(rows - 1)) : var;
    float om = 1.f - decay;
    mm[col] = mm[col] - (mm[col] - (float)mu) * om;
    mv[col] = mv[col] - (mv[col] - (float)uvar) * om;
  }
}

template <typename T>
__global__ void bn_apply_fwd_kernel(long total, int rows_per_sample, int c, const T* x, const int32_t* labels,
                                    const float* gamma, const float* beta, const float* mean, const float* rstd, int act, T* y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int ch = (int)(i % c);
    long row = i / c;
    int l = labels ? labels[row / rows_per_sample] : 0;
    // tf.nn.batch_normalization: inv = rsqrt(var+eps)*scale; y = x*inv + (offset - mean*inv)
    float inv = rstd[ch] * gamma[(long)l * c + ch];
    float v = Elem<T>::ld(x + i) * inv + (beta[(long)l * c + ch] - mean[ch] * inv);
    Elem<T>::st(y + i, act_apply(act, v));
  }
}

// combine the per-group backward partials: dgamma/dbeta per label and the two batch-wide sums
__global__ void bn_bwd_combine_kernel(int c, int ngroups, int n_labels, const int32_t* group_labels, const float* gamma,
                                      const float* partial, float* dgamma, float* dbeta, float* s12, int accumulate) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= c) return;
  double db[MAX_LABELS], dg[MAX_LABELS];
  for (int l = 0; l < MAX_LABELS; ++l) { db[l] = 0.0; dg[l] = 0.0; }
  for (int g = 0; g < ngroups; ++g) {
    int l = group_labels ? group_labels[g] : 0;
    db[l] += (double)partial[((long)g * 2 + 0) * c + col];
    dg[l] += (double)partial[((long)g * 2 + 1) * c + col];
  }
  double s1 = 0.0, s2 = 0.0;
  for (int l = 0; l < n_labels; ++l) {
    double gm = (double)gamma[(long)l * c + col];
    s1 += gm * db[l];
    s2 += gm * dg[l];
    float og = (float)dg[l], ob = (float)db[l];
    if (accumulate) { og += dgamma[(long)l * c + col]; ob += dbeta[(long)l * c + col]; }
    dgamma[(long)l * c + col] = og;
    dbeta[(long)l * c + col] = ob;
  }
  s12[col] = (float)s1;
  s12[c + col] = (float)s2;
}

template <typename T>
__global__ void bn_bwd_apply_kernel(long total, long rows, int rows_per_sample, int c, const T* x, const T* y, const T* dy,
                                    const int32_t* labels, const float* gamma, const float* mean, const float* rstd,
                                    const float* s12, int act, T* dx, int accumulate_dx) {
  const float invM = 1.f / (float)rows;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int ch = (int)(i % c);
    long row = i / c;
    int l = labels ? labels[row / rows_per_sample] : 0;
    float g = Elem<T>::ld(dy + i);
    if (act != RCGAN_ACT_NONE) g *= act_grad(act, Elem<T>::ld(y + i));
    float rs = rstd[ch];
    float xh = (Elem<T>::ld(x + i) - mean[ch]) * rs;
    float dxh = g * gamma[(long)l * c + ch];
    float v = rs * (dxh - s12[ch] * invM - xh * s12[c + ch] * invM);
    if (accumulate_dx) v += Elem<T>::ld(dx + i);
    Elem<T>::st(dx + i, v);
  }
}

// dx (=|+=) dy * act'(y) * gamma / sqrt(moving_var + eps): the adjoint of bn_infer w.r.t. its input (statistics and
// affine parameters are constants of the frozen sampler, mnist/model.py:494-640 recover_labels)
template <typename T>
__global__ void bn_infer_bwd_kernel(long total, int c, const T* y, const T* dy, const float* gamma, const float* mv, float eps, int act,
                                    T* dx, int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    float g = Elem<T>::ld(dy + i);
    if (act != RCGAN_ACT_NONE) g *= act_grad(act, Elem<T>::ld(y + i));
    float v = g * gamma[ch] / sqrtf(mv[ch] + eps);
    if (accumulate) v += Elem<T>::ld(dx + i);
    Elem<T>::st(dx + i, v);
  }
}

template <typename T>
__global__ void bn_infer_kernel(long total, int c, const T* x, const float* gamma, const float* beta, const float* mm,
                                const float* mv, float eps, int act, T* y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int ch = (int)(i % c);
    float v = (Elem<T>::ld(x + i) - mm[ch]) / sqrtf(mv[ch] + eps) * gamma[ch] + beta[ch];
    Elem<T>::st(y + i, act_apply(act, v));
  }
}


// ------------------------------------------------------------------------------------------------
// 8-wide vectorised variants (c % 8 == 0): one 16-B (bf16) / two 16-B (fp32) accesses per thread per row
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ld8(const float* p, float* v) {
  float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8(const bf16_t* p, float* v) {
  uint4 a = *(const uint4*)p;
  uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[2 * j] = bf16_to_f32((bf16_t)(w[j] & 0xffff)); v[2 * j + 1] = bf16_to_f32((bf16_t)(w[j] >> 16)); }
}
__device__ __forceinline__ void st8(float* p, const float* v) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void st8(bf16_t* p, const float* v) {
  uint4 pk;
  pk.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  pk.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
  pk.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
  pk.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
  *(uint4*)p = pk;
}

// block = 32 channel-chunks (256 channels) x 8 row lanes; grid = (ceil(chunks/32), groups)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_partial_vec_kernel(long rows, int c, long rows_per_group, const T* x, const T* y,
                                                             const T* dy, const float* mean, const float* rstd, int act,
                                                             float* partial) {
  __shared__ float red[2][8][256];
  const int chunk = blockIdx.x * 32 + (threadIdx.x & 31);
  const int rl = threadIdx.x >> 5;
  const bool on = chunk * 8 < c;
  const long rb = (long)blockIdx.y * rows_per_group;
  long re = rb + rows_per_group;
  if (re > rows) re = rows;
  float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; mu[j] = 0.f; rs[j] = 1.f; }
  if (on) {
    if (MODE == 1) { ld8(mean + chunk * 8, mu); ld8(rstd + chunk * 8, rs); }
#pragma unroll 2
    for (long r = rb + rl; r < re; r += 8) {
      const long off = r * c + chunk * 8;
      float xv[8];
      ld8(x + off, xv);
      if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += xv[j]; s2[j] += xv[j] * xv[j]; }
      } else {
        float gv[8], yv[8];
        ld8(dy + off, gv);
        if (act != RCGAN_ACT_NONE) {
          ld8(y + off, yv);
#pragma unroll
          for (int j = 0; j < 8; ++j) gv[j] *= act_grad(act, yv[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += gv[j]; s2[j] += gv[j] * (xv[j] - mu[j]) * rs[j]; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][rl][(threadIdx.x & 31) * 8 + j] = s1[j];
    red[1][rl][(threadIdx.x & 31) * 8 + j] = s2[j];
  }
  __syncthreads();
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col < c) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { a += red[0][q][threadIdx.x]; b += red[1][q][threadIdx.x]; }
    partial[((long)blockIdx.y * 2 + 0) * c + col] = a;
    partial[((long)blockIdx.y * 2 + 1) * c + col] = b;
  }
}

// per-(label, channel) affine of the forward: A = rstd*gamma, B = beta - mean*A   (tf.nn.batch_normalization)
__global__ void bn_table_fwd_kernel(int n_labels, int c, const float* gamma, const float* beta, const float* mean,
                                    const float* rstd, float* A, float* B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_labels * c) return;
  int ch = i % c;
  float a = rstd[ch] * gamma[i];
  A[i] = a;
  B[i] = beta[i] - mean[ch] * a;
}

// backward constants: A = rstd*gamma [labels][c];  dx = A*g + P*x + Q with P = -rstd^2*s2/M, Q = -P*mean - rstd*s1/M
__global__ void bn_table_bwd_kernel(int n_labels, int c, long rows, const float* gamma, const float* mean, const float* rstd,
                                    const float* s12, float* A, float* PQ) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_labels * c) A[i] = rstd[i % c] * gamma[i];
  if (i < c) {
    const float invM = 1.f / (float)rows;
    float rs = rstd[i];
    float p = -rs * rs * s12[c + i] * invM;
    PQ[i] = p;
    PQ[c + i] = -p * mean[i] - rs * s12[i] * invM;
  }
}

template <typename T>
__global__ void bn_apply_vec_kernel(long nchunks, int rows_per_sample, int c, const T* x, const int32_t* labels,
                                    const float* A, const float* B, int act, T* y) {
  const int cpr = c / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpr) * 8;
    const long row = i / cpr;
    const int l = labels ? labels[row / rows_per_sample] : 0;
    float xv[8], a[8], b[8];
    ld8(x + row * c + ch, xv);
    ld8(A + (long)l * c + ch, a);
    ld8(B + (long)l * c + ch, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[j] = act_apply(act, xv[j] * a[j] + b[j]);
    st8(y + row * c + ch, xv);
  }
}

template <typename T>
__global__ void bn_bwd_apply_vec_kernel(long nchunks, int rows_per_sample, int c, const T* x, const T* y, const T* dy,
                                        const int32_t* labels, const float* A, const float* PQ, int act, T* dx, int accumulate_dx) {
  const int cpr = c / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpr) * 8;
    const long row = i / cpr;
    const int l = labels ? labels[row / rows_per_sample] : 0;
    const long off = row * c + ch;
    float xv[8], gv[8], a[8], p[8], q[8];
    ld8(x + off, xv);
    ld8(dy + off, gv);
    if (act != RCGAN_ACT_NONE) {
      float yv[8];
      ld8(y + off, yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) gv[j] *= act_grad(act, yv[j]);
    }
    ld8(A + (long)l * c + ch, a);
    ld8(PQ + ch, p);
    ld8(PQ + c + ch, q);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = a[j] * gv[j] + p[j] * xv[j] + q[j];
    if (accumulate_dx) {
      float d[8];
      ld8(dx + off, d);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += d[j];
    }
    st8(dx + off, o);
  }
}

// ------------------------------------------------------------------------------------------------
// Fused variants (c % 64 == 0): statistics and their combination in ONE launch, affine tables folded into
// the apply kernels -> 2 launches per batch norm (was 4) in each direction.
//   * grid (c/64, groups); block = 8 channel chunks (64 channels) x 32 row lanes
//   * every workgroup writes its group's partial sums with agent-scope stores, then bumps an arrival counter of
//     its column block; the LAST arrival of a column block combines all groups of these 64 channels in a fixed
//     order (deterministic, fp64) and resets the counter for the next launch / graph replay.  Agent-scope
//     accesses go to the memory side, so no workgroup pays an L2 write-back/invalidate (8 XCDs = 8 L2s).
// ------------------------------------------------------------------------------------------------
// The affine part of batch norm as ONE fixed sequence of fp32 operations -- inv = rstd*gamma, c0 = fma(-mean, inv, beta),
// pre = fma(x, inv, c0) -- shared by the forward apply kernel and the backward kernels: the backward pass can then recompute
// the sign of the pre-activation (the ReLU / leaky-ReLU mask) from x bit-exactly instead of reading y a second and third time
// (y = act(pre) rounded to 16 bits has the sign of pre: bf16 / fp16 rounding keeps it, underflow to zero aside).
__device__ __forceinline__ float bn_pre(float x, float inv, float c0) { return __fmaf_rn(x, inv, c0); }
// ... rounded the way the forward stored act(pre): the recomputed mask is then bit-identical to one read from y, including the
// pre-activations that underflow to zero in fp16 (0 < pre < 2^-25; seen once in 4M elements in the parity tests)
template <typename T> __device__ __forceinline__ float bn_stored(float v);
template <> __device__ __forceinline__ float bn_stored<float>(float v) { return v; }
template <> __device__ __forceinline__ float bn_stored<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }
__device__ __forceinline__ float bn_c0(float mean, float inv, float beta) { return __fmaf_rn(-mean, inv, beta); }

__device__ __forceinline__ float ld_sc1_f1(__amdgpu_buffer_rsrc_t rs, unsigned byte_off, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, byte_off, soff, 16));
}

struct BnFusedArgs {
  long rows; int c; long rows_per_group; int ngroups;
  int nseg;                             // forward only: blockIdx.z = segment; x, partial, counter, mean, rstd advance per segment
  const void *x, *y, *dy;
  const float *mean_in, *rstd_in;       // backward only
  int act;
  float* partial;                       // [ngroups][2][c]
  unsigned* counter;                    // [c/64]
  // forward finish
  float eps; float *mean, *rstd, *mm, *mv; float decay;
  // backward finish
  int n_labels; int groups_per_sample; const int32_t* labels; int n_samples;
  const float* gamma; float *dgamma, *dbeta; int accumulate; float* PQ;
  const float* beta;                    // backward, optional: with it the activation mask is recomputed from x (no read of y)
  int nsub;                             // conditional backward, samples of < 32 rows: a workgroup takes 32 rows = nsub samples (0, 1: off)
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_fused_reduce_kernel(BnFusedArgs a) {
  // dynamic LDS: the row buffer red[2][32][64] of the streaming phase; the finisher of the conditional backward reuses it as
  // lacc[2][n_labels][4][64] (per-label sums, private per (lane4, column)).  Sharing the storage (16 KiB, 20 KiB with ten labels,
  // instead of 60 KiB of static arrays) is what lets six workgroups instead of two stay on a CU: this kernel is a latency chain
  // (load -> LDS -> write-through store -> arrival), so its time is rounds x chain.
  extern __shared__ float uni[];
  __shared__ double fin[2][4][64];
  __shared__ float lab_s[2][64];
  __shared__ int is_last;
  __shared__ int lab_ids[128];
#define RED(k, q, col) uni[((k) * 32 + (q)) * 64 + (col)]
#define LACC(k, l, ln, col) uni[(((k) * NL + (l)) * 4 + (ln)) * 64 + (col)]
  const int NL = a.n_labels;
  const int nsub = a.nsub > 1 ? a.nsub : 1;     // samples per workgroup when a sample has fewer than 32 rows
  const int t = threadIdx.x;
  const int c = a.c;
  const int c0 = blockIdx.x * 64;
  const int chunk = t & 7, rl = t >> 3;
  const long rb = (long)blockIdx.y * a.rows_per_group;
  long re = rb + a.rows_per_group;
  if (re > a.rows) re = a.rows;
  if (MODE == 0 && a.nseg > 1) {        // independent statistics per segment of a.rows rows (batched generator forward)
    const long sg = blockIdx.z;
    a.x = (const T*)a.x + sg * a.rows * c;
    a.partial += sg * (long)a.ngroups * 2 * c;
    a.counter += sg * (c / 64) * RC_LINE_STRIDE;
    a.mean += sg * c; a.rstd += sg * c;
  }
  const T* x = (const T*)a.x; const T* y = (const T*)a.y; const T* dy = (const T*)a.dy;
  float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; mu[j] = 0.f; rs[j] = 1.f; }
  float ainv[8], ac0[8];
  const bool mask_x = MODE == 1 && a.beta != nullptr;
  constexpr int UNR = MODE == 0 ? 4 : 2;
  if (MODE == 1) { ld8(a.mean_in + c0 + chunk * 8, mu); ld8(a.rstd_in + c0 + chunk * 8, rs); }
  if (mask_x) {                           // the group's rows belong to one sample: one label
    const int smp = nsub > 1 ? (int)blockIdx.y * nsub + rl / (32 / nsub) : (int)blockIdx.y / a.groups_per_sample;
    const long lo = (long)(a.labels ? a.labels[smp] : 0) * c + c0 + chunk * 8;
    float gm8[8], bt8[8];
    ld8(a.gamma + lo, gm8); ld8(a.beta + lo, bt8);
#pragma unroll
    for (int j = 0; j < 8; ++j) { ainv[j] = rs[j] * gm8[j]; ac0[j] = bn_c0(mu[j], ainv[j], bt8[j]); }
  }
#pragma unroll UNR
  for (long r = rb + rl; r < re; r += 32) {
    const long off = r * c + c0 + chunk * 8;
    float xv[8];
    ld8(x + off, xv);
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += xv[j]; s2[j] += xv[j] * xv[j]; }
    } else {
      float gv[8];
      ld8(dy + off, gv);
      if (mask_x) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(a.act, bn_stored<T>(bn_pre(xv[j], ainv[j], ac0[j])));
      } else if (a.act != RCGAN_ACT_NONE) {
        float yv[8];
        ld8(y + off, yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(a.act, yv[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += gv[j]; s2[j] += gv[j] * (xv[j] - mu[j]) * rs[j]; }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { RED(0, rl, chunk * 8 + j) = s1[j]; RED(1, rl, chunk * 8 + j) = s2[j]; }
  __syncthreads();
  // wavefront 0 writes both partial rows and then signals: the agent-scope release of thread 0 orders the
  // stores of its OWN wavefront, so no other wavefront has to fence
  if (t < 64) {
    const int qn = 32 / nsub;
    for (int sub = 0; sub < nsub; ++sub) {
      float sa = 0.f, sb = 0.f;
#pragma unroll 8
      for (int q = sub * qn; q < (sub + 1) * qn; ++q) { sa += RED(0, q, t); sb += RED(1, q, t); }
      // agent-scope stores (write through to the memory side: visible to every XCD without an L2 write-back)
      const long pr = (long)blockIdx.y * nsub + sub;
      __hip_atomic_store(a.partial + (pr * 2 + 0) * c + c0 + t, sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.partial + (pr * 2 + 1) * c + c0 + t, sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's stores are performed before it signals
  }
  // ---- arrival: the last workgroup of this column block finishes ------------------------------------------
  if (t == 0) {
    unsigned prev = __hip_atomic_fetch_add(a.counter + blockIdx.x * RC_LINE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = (prev == (unsigned)a.ngroups - 1u) ? 1 : 0;
  }
  __syncthreads();
  if (!is_last) return;
  // the partials are read back with agent-scope loads (served from the memory side, never from a stale cache line)
  const int col = t & 63, lane4 = t >> 6;
  const float* part = a.partial + c0 + col;
  const long gstride = 2L * c;

  if (MODE == 0 || a.labels == nullptr) {
    double d1 = 0.0, d2 = 0.0;
#pragma unroll 8
    for (int g = lane4; g < a.ngroups; g += 4) {
      d1 += (double)__hip_atomic_load(part + g * gstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      d2 += (double)__hip_atomic_load(part + g * gstride + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    fin[0][lane4][col] = d1; fin[1][lane4][col] = d2;
    __syncthreads();
    if (t < 64) {
      d1 = fin[0][0][t] + fin[0][1][t] + fin[0][2][t] + fin[0][3][t];
      d2 = fin[1][0][t] + fin[1][1][t] + fin[1][2][t] + fin[1][3][t];
      const int ch = c0 + t;
      if (MODE == 0) {
        double mean = d1 / (double)a.rows;
        double var = d2 / (double)a.rows - mean * mean;
        if (var < 0.0) var = 0.0;
        a.mean[ch] = (float)mean;
        a.rstd[ch] = (float)(1.0 / sqrt(var + (double)a.eps));
        if (a.mm) {
          // TF fused batch norm: moving -= (moving - batch) * (1 - decay), variance with Bessel's correction
          double uvar = a.rows > 1 ? var * ((double)a.rows / (double)(a.rows - 1)) : var;
          float om = 1.f - a.decay;
          a.mm[ch] = a.mm[ch] - (a.mm[ch] - (float)mean) * om;
          a.mv[ch] = a.mv[ch] - (a.mv[ch] - (float)uvar) * om;
        }
      } else {
        float og = (float)d2, ob = (float)d1;
        if (a.accumulate) { og += a.dgamma[ch]; ob += a.dbeta[ch]; }
        a.dgamma[ch] = og; a.dbeta[ch] = ob;
        lab_s[0][t] = (float)d1; lab_s[1][t] = (float)d2;
      }
    }
  } else {
    // conditional: the groups of one sample are contiguous.  Thread (column, lane4) owns samples lane4*8..+7 of
    // every batch of 32: it sums their groups (independent loads) and adds the result to its PRIVATE per-label
    // slot in LDS; afterwards the four lanes of a (label, column) are summed in a fixed order.
    const int gps = a.groups_per_sample;
    for (int l = 0; l < NL; ++l) { LACC(0, l, lane4, col) = 0.f; LACC(1, l, lane4, col) = 0.f; }
    // FB*32 samples per round: FB*16 independent loads per thread and group; buffer loads (one 32-bit offset per sample, the
    // second row through the scalar offset; samples past the end read zero).  Measured: 64 samples per round 3 us faster than
    // 128 (142 VGPRs), and than 32 with 64-bit addresses
    constexpr int FB = 2;
    const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc((void*)a.partial, 0, (int)((long)a.n_samples * gps * gstride * 4), 0x00020000);
    const unsigned sstride = (unsigned)(gps * gstride * 4);
    for (int s0 = 0; s0 < a.n_samples; s0 += FB * 32) {
      __syncthreads();
      int lab = -1;
      if (t < FB * 32 && s0 + t < a.n_samples) lab = a.labels[s0 + t];
      float d1[FB][8], d2[FB][8];
#pragma unroll
      for (int b = 0; b < FB; ++b)
#pragma unroll
        for (int k = 0; k < 8; ++k) { d1[b][k] = 0.f; d2[b][k] = 0.f; }
      for (int q = 0; q < gps; ++q) {
        const unsigned o0 = (unsigned)(c0 + col) * 4u + (unsigned)q * (unsigned)(gstride * 4);
#pragma unroll
        for (int b = 0; b < FB; ++b) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const unsigned o = o0 + (unsigned)(s0 + b * 32 + lane4 * 8 + k) * sstride;
            d1[b][k] += ld_sc1_f1(rs_p, o, 0);
            d2[b][k] += ld_sc1_f1(rs_p, o, c * 4);
          }
        }
      }
      if (t < FB * 32) lab_ids[t] = lab;
      __syncthreads();
#pragma unroll
      for (int b = 0; b < FB; ++b) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int l = lab_ids[b * 32 + lane4 * 8 + k];
          if (l >= 0 && l < NL) { LACC(0, l, lane4, col) += d1[b][k]; LACC(1, l, lane4, col) += d2[b][k]; }
        }
      }
    }
    __syncthreads();
    double q1 = 0.0, q2 = 0.0;
#pragma unroll
    for (int slot = 0; slot < MAX_LABELS / 4; ++slot) {
      const int l = lane4 + 4 * slot;
      if (l < NL) {
        const float acc1 = (LACC(0, l, 0, col) + LACC(0, l, 1, col)) + (LACC(0, l, 2, col) + LACC(0, l, 3, col));
        const float acc2 = (LACC(1, l, 0, col) + LACC(1, l, 1, col)) + (LACC(1, l, 2, col) + LACC(1, l, 3, col));
        const long o = (long)l * c + c0 + col;
        const float gm = a.gamma[o];
        float og = acc2, ob = acc1;
        if (a.accumulate) { og += a.dgamma[o]; ob += a.dbeta[o]; }
        a.dgamma[o] = og; a.dbeta[o] = ob;
        q1 += (double)gm * (double)acc1;
        q2 += (double)gm * (double)acc2;
      }
    }
    fin[0][lane4][col] = q1; fin[1][lane4][col] = q2;
  }
  if (MODE == 1) {
    __syncthreads();
    if (t < 64) {
      // dx = A*g + P*x + Q with A = rstd*gamma[label], P = -rstd^2*s2/M, Q = -P*mean - rstd*s1/M,
      // s1 = sum_l gamma_l*dbeta_l, s2 = sum_l gamma_l*dgamma_l
      const int ch = c0 + t;
      double q1, q2;
      if (a.labels == nullptr) {
        const double gmm = (double)a.gamma[ch];
        q1 = gmm * (double)lab_s[0][t]; q2 = gmm * (double)lab_s[1][t];
      } else {
        q1 = fin[0][0][t] + fin[0][1][t] + fin[0][2][t] + fin[0][3][t];
        q2 = fin[1][0][t] + fin[1][1][t] + fin[1][2][t] + fin[1][3][t];
      }
      const float invM = 1.f / (float)a.rows;
      const float r = a.rstd_in[ch];
      const float p = -r * r * (float)q2 * invM;
      a.PQ[ch] = p;
      a.PQ[c + ch] = -p * a.mean_in[ch] - r * (float)q1 * invM;
    }
  }
  if (t == 0) __hip_atomic_store(a.counter + blockIdx.x * RC_LINE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#undef RED
#undef LACC
}

// ------------------------------------------------------------------------------------------------
// Tree variant of the fused reduction for LARGE tensors (>= a few MB).  The kernel above gives every workgroup a 64-channel
// column block: 128 bytes out of every 512-byte (c = 256) row, with the other three quarters of the row read by workgroups
// on other XCDs at other times -- measured 2.5-2.9 TB/s where the contiguous apply kernels reach 5-6.  Here a workgroup
// streams WHOLE rows (rows_per_group x c contiguous bytes), and because every workgroup then holds partial sums of every
// channel, the combination is a two-level arrival tree instead of "last workgroup of the column":
//   level 1: groups are dealt to clusters (16 consecutive groups; backward with labels: the groups of one sample).  The
//            last group of a cluster to arrive adds the cluster's partials in group order -> cpart[cluster][2][c] (fp64).
//   level 2: the last cluster to finish adds the cluster partials in cluster order (per label for the conditional
//            backward) and writes mean / rstd (or dgamma / dbeta / P,Q).
// Every sum has a fixed order: results are bit-reproducible.  Partials travel with agent-scope (write-through) stores and
// loads; counters reset themselves (graph replay).
// ------------------------------------------------------------------------------------------------
struct BnTreeArgs {
  BnFusedArgs f;             // partial = [ngroups][2c] fp32
  float* cpart;              // [nclusters][2c]
  unsigned* counters;        // [nclusters] + [1]   (per segment)
  int cs, nclusters;         // groups per cluster
};

typedef unsigned int v4u32 __attribute__((__vector_size__(16)));
// 16-byte agent-scope (sc1) accesses: served by / written through to the memory side, never a stale or dirty line of an XCD's L2
__device__ __forceinline__ float4 ld_sc1_f4(__amdgpu_buffer_rsrc_t rs, unsigned byte_off) {
  const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 16);
  const unsigned e0 = v[0], e1 = v[1], e2 = v[2], e3 = v[3];     // (named scalars: __builtin_bit_cast of a vector ELEMENT reads element 0)
  return make_float4(__builtin_bit_cast(float, e0), __builtin_bit_cast(float, e1), __builtin_bit_cast(float, e2), __builtin_bit_cast(float, e3));
}
__device__ __forceinline__ void st_sc1_f4(__amdgpu_buffer_rsrc_t rs, unsigned byte_off, float4 f) {
  const v4u32 v = {__builtin_bit_cast(unsigned, f.x), __builtin_bit_cast(unsigned, f.y), __builtin_bit_cast(unsigned, f.z), __builtin_bit_cast(unsigned, f.w)};
  __builtin_amdgcn_raw_buffer_store_b128(v, rs, byte_off, 0, 16);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_tree_reduce_kernel(BnTreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) float tsm[];
  __shared__ int flag;
  BnFusedArgs& a = ta.f;
  const int t = threadIdx.x;
  const int c = a.c, c2 = 2 * c;
  const int cpr = c >> 3, lcpr = __ffs(cpr) - 1;
  const int chunk = t & (cpr - 1), rl = t >> lcpr, RL = 256 >> lcpr;
  const int g = blockIdx.x;
  const long rb = (long)g * a.rows_per_group;
  long re = rb + a.rows_per_group;
  if (re > a.rows) re = a.rows;
  if (MODE == 0 && a.nseg > 1) {
    const long sg = blockIdx.y;
    a.x = (const T*)a.x + sg * a.rows * c;
    a.partial += sg * (long)a.ngroups * c2;
    ta.cpart += sg * (long)ta.nclusters * c2;
    ta.counters += sg * (ta.nclusters + 1) * RC_LINE_STRIDE;
    a.mean += sg * c; a.rstd += sg * c;
  }
  const T* x = (const T*)a.x; const T* y = (const T*)a.y; const T* dy = (const T*)a.dy;
  float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; mu[j] = 0.f; rs[j] = 1.f; }
  float ainv[8], ac0[8];
  const bool mask_x = MODE == 1 && a.beta != nullptr;
  if (MODE == 1) { ld8(a.mean_in + chunk * 8, mu); ld8(a.rstd_in + chunk * 8, rs); }
  if (mask_x) {
    const long lo = (long)(a.labels ? a.labels[g / a.groups_per_sample] : 0) * c + chunk * 8;
    float gm8[8], bt8[8];
    ld8(a.gamma + lo, gm8); ld8(a.beta + lo, bt8);
#pragma unroll
    for (int j = 0; j < 8; ++j) { ainv[j] = rs[j] * gm8[j]; ac0[j] = bn_c0(mu[j], ainv[j], bt8[j]); }
  }
#pragma unroll 4
  for (long r = rb + rl; r < re; r += RL) {
    const long off = r * c + chunk * 8;
    float xv[8];
    ld8(x + off, xv);
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += xv[j]; s2[j] += xv[j] * xv[j]; }
    } else {
      float gv[8];
      ld8(dy + off, gv);
      if (mask_x) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(a.act, bn_stored<T>(bn_pre(xv[j], ainv[j], ac0[j])));
      } else if (a.act != RCGAN_ACT_NONE) {
        float yv[8];
        ld8(y + off, yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(a.act, yv[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += gv[j]; s2[j] += gv[j] * (xv[j] - mu[j]) * rs[j]; }
    }
  }
  // ---- workgroup partial: sum over the row lanes through LDS ([2][RL][c] floats), written through as [2c] ----------
  float* red = tsm;
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[(0 * RL + rl) * c + chunk * 8 + j] = s1[j]; red[(1 * RL + rl) * c + chunk * 8 + j] = s2[j]; }
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rs_part = __builtin_amdgcn_make_buffer_rsrc(a.partial, 0, (int)((long)a.ngroups * c2 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_cp = __builtin_amdgcn_make_buffer_rsrc(ta.cpart, 0, (int)((long)ta.nclusters * c2 * 4), 0x00020000);
  const int Q = c2 >> 2;                                     // 16-byte quads of one partial row
  for (int qd = t; qd < Q; qd += 256) {
    const int q = qd * 4 >= c ? 1 : 0, ch = qd * 4 - q * c;
    float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < RL; ++k) {
      const float4 v = *(const float4*)(red + (q * RL + k) * c + ch);
      sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
    }
    st_sc1_f4(rs_part, (unsigned)(((long)g * c2 + qd * 4) * 4), sm);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wavefront drains its write-through stores ...
  __syncthreads();                                           // ... before one lane signals
  const int cl = g / ta.cs;
  const int cl_groups = min(ta.cs, a.ngroups - cl * ta.cs);
  if (t == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ta.counters + cl * RC_LINE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag = (prev == (unsigned)cl_groups - 1u) ? 1 : 0;
  }
  __syncthreads();
  if (!flag) return;
  // ---- level 1: this workgroup closes its cluster: cpart[cl] = sum of its groups' partials, in group order ------------
  for (int qd = t; qd < Q; qd += 256) {
    float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned base = (unsigned)(((long)cl * ta.cs * c2 + qd * 4) * 4);
#pragma unroll 16
    for (int k = 0; k < cl_groups; ++k) {
      const float4 v = ld_sc1_f4(rs_part, base + (unsigned)k * (unsigned)c2 * 4u);
      sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
    }
    st_sc1_f4(rs_cp, (unsigned)(((long)cl * c2 + qd * 4) * 4), sm);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    __hip_atomic_store(ta.counters + cl * RC_LINE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned prev = __hip_atomic_fetch_add(ta.counters + ta.nclusters * RC_LINE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag = (prev == (unsigned)ta.nclusters - 1u) ? 1 : 0;
  }
  __syncthreads();
  if (!flag) return;
  // ---- level 2: the last cluster to finish closes the reduction --------------------------------------------------------
  const bool cond = MODE == 1 && a.labels != nullptr;
  const int ncl = ta.nclusters;
  if (!cond) {
    double* fin = (double*)tsm;                              // [2c]
    for (int qd = t; qd < Q; qd += 256) {
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
#pragma unroll 16
      for (int k = 0; k < ncl; ++k) {
        const float4 v = ld_sc1_f4(rs_cp, (unsigned)(((long)k * c2 + qd * 4) * 4));
        d0 += (double)v.x; d1 += (double)v.y; d2 += (double)v.z; d3 += (double)v.w;
      }
      fin[qd * 4 + 0] = d0; fin[qd * 4 + 1] = d1; fin[qd * 4 + 2] = d2; fin[qd * 4 + 3] = d3;
    }
    __syncthreads();
    for (int ch = t; ch < c; ch += 256) {
      const double d1 = fin[ch], d2 = fin[c + ch];
      if (MODE == 0) {
        const double mean = d1 / (double)a.rows;
        double var = d2 / (double)a.rows - mean * mean;
        if (var < 0.0) var = 0.0;
        a.mean[ch] = (float)mean;
        a.rstd[ch] = (float)(1.0 / sqrt(var + (double)a.eps));
        if (a.mm) {
          const double uvar = a.rows > 1 ? var * ((double)a.rows / (double)(a.rows - 1)) : var;
          const float om = 1.f - a.decay;
          a.mm[ch] = a.mm[ch] - (a.mm[ch] - (float)mean) * om;
          a.mv[ch] = a.mv[ch] - (a.mv[ch] - (float)uvar) * om;
        }
      } else {
        float og = (float)d2, ob = (float)d1;
        if (a.accumulate) { og += a.dgamma[ch]; ob += a.dbeta[ch]; }
        a.dgamma[ch] = og; a.dbeta[ch] = ob;
        const double gmm = (double)a.gamma[ch];
        const float invM = 1.f / (float)a.rows;
        const float r = a.rstd_in[ch];
        const float p = -r * r * (float)(gmm * d2) * invM;
        a.PQ[ch] = p;
        a.PQ[c + ch] = -p * a.mean_in[ch] - r * (float)(gmm * d1) * invM;
      }
    }
  } else {
    // conditional backward: cluster = sample.  Thread (quad, sample lane) bins its samples' partial rows by label into
    // lacc[SL][n_labels][2c] (LDS; every (lane, quad) column is private to one thread), then a thread per channel adds the
    // lanes in order.
    const int nl = a.n_labels;
    const int SL = Q >= 256 ? 1 : 256 / Q;
    float* lacc = tsm;
    for (int i = t; i < SL * nl * c2; i += 256) lacc[i] = 0.f;
    __syncthreads();
    const int sl = Q >= 256 ? 0 : t / Q;
    for (int qd = Q >= 256 ? t : t - sl * Q; qd < Q; qd += 256) {
      for (int s0 = sl; s0 < ncl; s0 += SL * 16) {
        float4 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int s = s0 + k * SL;
          v[k] = s < ncl ? ld_sc1_f4(rs_cp, (unsigned)(((long)s * c2 + qd * 4) * 4)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int s = s0 + k * SL;
          if (s < ncl) {
            const int l = a.labels[s];
            if (l >= 0 && l < nl) {
              float4* dst = (float4*)(lacc + ((long)sl * nl + l) * c2 + qd * 4);
              float4 o = *dst;
              o.x += v[k].x; o.y += v[k].y; o.z += v[k].z; o.w += v[k].w;
              *dst = o;
            }
          }
        }
      }
    }
    __syncthreads();
    for (int ch = t; ch < c; ch += 256) {
      double q1 = 0.0, q2 = 0.0;
      for (int l = 0; l < nl; ++l) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < SL; ++k) { a1 += lacc[((long)k * nl + l) * c2 + ch]; a2 += lacc[((long)k * nl + l) * c2 + c + ch]; }
        const long o = (long)l * c + ch;
        float og = a2, ob = a1;
        if (a.accumulate) { og += a.dgamma[o]; ob += a.dbeta[o]; }
        a.dgamma[o] = og; a.dbeta[o] = ob;
        const double gm = (double)a.gamma[o];
        q1 += gm * (double)a1;
        q2 += gm * (double)a2;
      }
      const float invM = 1.f / (float)a.rows;
      const float r = a.rstd_in[ch];
      const float p = -r * r * (float)q2 * invM;
      a.PQ[ch] = p;
      a.PQ[c + ch] = -p * a.mean_in[ch] - r * (float)q1 * invM;
    }
  }
  if (t == 0) __hip_atomic_store(ta.counters + ta.nclusters * RC_LINE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// y = act(x*A + B), A = rstd*gamma[label], B = beta[label] - mean*A, computed in-line: the thread's 8 channels are fixed
// (grid stride is a multiple of the chunks per row), so mean/rstd live in registers.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_fused_kernel(long nchunks, int rows_per_sample, int c, const T* x, const int32_t* labels,
                                                             const float* gamma, const float* beta, const float* mean,
                                                             const float* rstd, int act, T* y, int n_per_seg) {
  if (gridDim.y > 1) {                                // blockIdx.y = segment: nchunks / n_per_seg count ONE segment
    const long sg = blockIdx.y;
    x += sg * nchunks * 8; y += sg * nchunks * 8;
    if (labels) labels += sg * n_per_seg;
    mean += sg * c; rstd += sg * c;
  }
  const unsigned cpr = (unsigned)c / 8u;              // a power of two on this path
  const int lcpr = __ffs((int)cpr) - 1;
  const int lrps = (rows_per_sample & (rows_per_sample - 1)) == 0 ? __ffs(rows_per_sample) - 1 : -1;
  const unsigned i0 = blockIdx.x * 256u + threadIdx.x;
  const unsigned stride = gridDim.x * 256u;
  const int ch = (int)(i0 & (cpr - 1u)) * 8;
  float mu[8], rs[8];
  ld8(mean + ch, mu); ld8(rstd + ch, rs);
  for (unsigned i = i0; i < (unsigned)nchunks; i += stride) {
    const unsigned row = i >> lcpr;
    const int l = labels ? labels[lrps >= 0 ? (row >> lrps) : (row / (unsigned)rows_per_sample)] : 0;
    float xv[8], g[8], b[8];
    ld8(x + (long)row * c + ch, xv);
    ld8(gamma + (long)l * c + ch, g);
    ld8(beta + (long)l * c + ch, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float inv = rs[j] * g[j];
      xv[j] = act_apply(act, bn_pre(xv[j], inv, bn_c0(mu[j], inv, b[j])));
    }
    st8(y + (long)row * c + ch, xv);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_fused_kernel(long nchunks, int rows_per_sample, int c, const T* x, const T* y, const T* dy,
                                                                 const int32_t* labels, const float* gamma, const float* rstd,
                                                                 const float* PQ, int act, T* dx, int accumulate_dx,
                                                                 const float* beta, const float* mean) {
  const unsigned cpr = (unsigned)c / 8u;              // a power of two on this path
  const int lcpr = __ffs((int)cpr) - 1;
  const int lrps = (rows_per_sample & (rows_per_sample - 1)) == 0 ? __ffs(rows_per_sample) - 1 : -1;
  const unsigned i0 = blockIdx.x * 256u + threadIdx.x;
  const unsigned stride = gridDim.x * 256u;
  const int ch = (int)(i0 & (cpr - 1u)) * 8;
  float rs[8], p[8], q[8], mu[8];
  ld8(rstd + ch, rs); ld8(PQ + ch, p); ld8(PQ + c + ch, q);
  const bool mask_x = beta != nullptr;      // activation mask from x (bn_pre) instead of a read of y
  if (mask_x) ld8(mean + ch, mu);
  for (unsigned i = i0; i < (unsigned)nchunks; i += stride) {
    const unsigned row = i >> lcpr;
    const int l = labels ? labels[lrps >= 0 ? (row >> lrps) : (row / (unsigned)rows_per_sample)] : 0;
    const long off = (long)row * c + ch;
    float xv[8], gv[8], gm[8];
    ld8(x + off, xv);
    ld8(dy + off, gv);
    ld8(gamma + (long)l * c + ch, gm);
    if (mask_x) {
      float bt[8];
      ld8(beta + (long)l * c + ch, bt);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float inv = rs[j] * gm[j];
        gv[j] *= act_grad(act, bn_stored<T>(bn_pre(xv[j], inv, bn_c0(mu[j], inv, bt[j]))));
      }
    } else if (act != RCGAN_ACT_NONE) {
      float yv[8];
      ld8(y + off, yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) gv[j] *= act_grad(act, yv[j]);
    }
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = rs[j] * gm[j] * gv[j] + p[j] * xv[j] + q[j];
    if (accumulate_dx) {
      float d[8];
      ld8(dx + off, d);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += d[j];
    }
    st8(dx + off, o);
  }
}

// mean / rstd of `nseg` segments from the per-tile column sums a convolution's epilogue left (conv_mfma8.hip): part[tile][c][2] =
// (sum, sum of squares) over the tile's 256 pixels.  Segment s owns the tiles [g * group_stride + s * tps, + tps) of every group g
// (one group, or the four phases of the sub-pixel form).  grid (c / 16, nseg) x 256 threads: 16 channels x 16 tile subsets, every
// thread's loads independent of one another (one memory round trip), all sums in a fixed order in fp64.
__global__ __launch_bounds__(256) void bn_tile_stats_finish_kernel(const float* __restrict__ part, int c, int tps, int ngroups, long group_stride,
                                                                   double inv_count, float eps, float* mean, float* rstd) {
  __shared__ double red[2][16][16];
  const int cl = threadIdx.x & 15, sub = threadIdx.x >> 4, ch = blockIdx.x * 16 + cl, sg = blockIdx.y;
  double s1 = 0.0, s2 = 0.0;
  for (int g = 0; g < ngroups; ++g) {
    const long t0 = (long)g * group_stride + (long)sg * tps;
    for (int tb = sub; tb < tps; tb += 16 * 8) {
      float2 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = tb + q * 16;
        v[q] = t < tps ? *(const float2*)(part + ((t0 + t) * c + ch) * 2) : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) { s1 += (double)v[q].x; s2 += (double)v[q].y; }
    }
  }
  red[0][sub][cl] = s1; red[1][sub][cl] = s2;
  __syncthreads();
  if (sub == 0) {
    double a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) { a1 += red[0][q][cl]; a2 += red[1][q][cl]; }
    const double mu = a1 * inv_count;
    double var = a2 * inv_count - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[(long)sg * c + ch] = (float)mu;
    rstd[(long)sg * c + ch] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

int bn_tile_stats_finish_launch(rcgan_ctx* ctx, const float* part, int c, int nseg, int tiles_per_seg, int ngroups, long group_stride,
                                double count, float eps, float* mean, float* rstd) {
  RC_REQUIRE(ctx, c % 16 == 0 && tiles_per_seg >= 1, "bad tile statistics layout");
  hipLaunchKernelGGL(bn_tile_stats_finish_kernel, dim3(c / 16, nseg), dim3(256), 0, ctx->stream, part, c, tiles_per_seg, ngroups, group_stride,
                     1.0 / count, eps, mean, rstd);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// ------------------------------------------------------------------------------------------------
// Conditional backward for MORE than MAX_LABELS classes (CIFAR-100: 100 or 20, 1000-class sets; up to BN_MAX_LABELS_WIDE).  The
// narrow paths keep per-label accumulators in registers or LDS; here nothing scales with the class count:
//   1. bn_sample_partial_kernel: one row group per sample -> partial[s][0][c] = sum dy', partial[s][1][c] = sum dy' * xhat
//   2. bn_bwd_class_kernel: workgroup row l < K walks the samples in index order and adds, in fp64, the partials of those whose
//      label is l -> dgamma[l] / dbeta[l] (an absent class gets exactly 0, or is left untouched under `accumulate`); row K
//      forms s1 = sum_s gamma[l_s] * partial[s][0], s2 likewise (fp64, sample order) and the dx constants PQ / s12.
//   3. the existing apply kernels (gamma[label] read per row, no K-sized table).
// No atomics: every sum has a fixed order, so results are bit-reproducible (graph replay).
// ------------------------------------------------------------------------------------------------

// block = 32 channel chunks (256 channels) x 8 row lanes; grid = (ceil(chunks / 32), n).  beta (optional): ReLU / leaky-ReLU
// mask recomputed from x with the forward's arithmetic (as bn_fused_reduce_kernel), y is then not read.
template <typename T>
__global__ __launch_bounds__(256) void bn_sample_partial_kernel(int rows_per_sample, int c, const T* x, const T* y, const T* dy,
                                                                const int32_t* labels, const float* gamma, const float* beta,
                                                                const float* mean, const float* rstd, int act, float* partial) {
  __shared__ float red[2][8][256];
  const int chunk = blockIdx.x * 32 + (threadIdx.x & 31);
  const int rl = threadIdx.x >> 5;
  const bool on = chunk * 8 < c;
  const long rb = (long)blockIdx.y * rows_per_sample, re = rb + rows_per_sample;
  float s1[8], s2[8], mu[8], rs[8], ainv[8], ac0[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  if (on) {
    ld8(mean + chunk * 8, mu); ld8(rstd + chunk * 8, rs);
    if (beta) {
      const long lo = (long)labels[blockIdx.y] * c + chunk * 8;
      float gm8[8], bt8[8];
      ld8(gamma + lo, gm8); ld8(beta + lo, bt8);
#pragma unroll
      for (int j = 0; j < 8; ++j) { ainv[j] = rs[j] * gm8[j]; ac0[j] = bn_c0(mu[j], ainv[j], bt8[j]); }
    }
#pragma unroll 2
    for (long r = rb + rl; r < re; r += 8) {
      const long off = r * c + chunk * 8;
      float xv[8], gv[8];
      ld8(x + off, xv);
      ld8(dy + off, gv);
      if (beta) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(act, bn_stored<T>(bn_pre(xv[j], ainv[j], ac0[j])));
      } else if (act != RCGAN_ACT_NONE) {
        float yv[8];
        ld8(y + off, yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] *= act_grad(act, yv[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1[j] += gv[j]; s2[j] += gv[j] * (xv[j] - mu[j]) * rs[j]; }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][rl][(threadIdx.x & 31) * 8 + j] = s1[j];
    red[1][rl][(threadIdx.x & 31) * 8 + j] = s2[j];
  }
  __syncthreads();
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col < c) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { a += red[0][q][threadIdx.x]; b += red[1][q][threadIdx.x]; }
    partial[((long)blockIdx.y * 2 + 0) * c + col] = a;
    partial[((long)blockIdx.y * 2 + 1) * c + col] = b;
  }
}

// grid (ceil(c / 256), K + 1) x 256 threads: a thread per channel; the labels pass through LDS 256 at a time
__global__ __launch_bounds__(256) void bn_bwd_class_kernel(int n, int c, int n_labels, long rows, const int32_t* labels, const float* gamma,
                                                           const float* partial, const float* mean, const float* rstd, float* dgamma,
                                                           float* dbeta, int accumulate, float* s12, float* PQ) {
  __shared__ int lab_s[256];
  const int t = threadIdx.x, ch = blockIdx.x * 256 + t, l = blockIdx.y;
  const bool totals = l == n_labels;
  double d1 = 0.0, d2 = 0.0;
  int cnt = 0;
  for (int s0 = 0; s0 < n; s0 += 256) {
    __syncthreads();
    if (s0 + t < n) lab_s[t] = labels[s0 + t];
    __syncthreads();
    const int m = min(256, n - s0);
    if (ch >= c) continue;
    for (int k = 0; k < m; ++k) {
      const int ls = lab_s[k];
      if (ls < 0 || ls >= n_labels || (!totals && ls != l)) continue;
      const float* pp = partial + (long)(s0 + k) * 2 * c + ch;
      if (totals) {
        const double gm = (double)gamma[(long)ls * c + ch];
        d1 += gm * (double)pp[0]; d2 += gm * (double)pp[c];
      } else {
        d1 += (double)pp[0]; d2 += (double)pp[c];
        ++cnt;
      }
    }
  }
  if (ch >= c) return;
  if (!totals) {
    if (cnt == 0 && accumulate) return;       // absent class: untouched
    const long o = (long)l * c + ch;
    float og = (float)d2, ob = (float)d1;
    if (accumulate) { og += dgamma[o]; ob += dbeta[o]; }
    dgamma[o] = og; dbeta[o] = ob;
    return;
  }
  s12[ch] = (float)d1;
  s12[c + ch] = (float)d2;
  // dx = A*g + P*x + Q, A = rstd*gamma[label] (read per row by the apply kernel), P = -rstd^2*s2/M, Q = -P*mean - rstd*s1/M
  const float invM = 1.f / (float)rows;
  const float r = rstd[ch];
  const float p = -r * r * (float)d2 * invM;
  PQ[ch] = p;
  PQ[c + ch] = -p * mean[ch] - r * (float)d1 * invM;
}

// ------------------------------------------------------------------------------------------------
// Host side.  bn_plan.h decides (bn_choose) and sizes (bn_plan) every launch, and holds the table of routes; here are the argument
// check, one launcher per kernel family and the entry points, each of which is: check, choose, plan, workspace check, launch.
// ------------------------------------------------------------------------------------------------
// the planner's limits against the counter layout of common.h (36864 / 102400: rcgan_ctx::line_counters / tree_line_counters)
static_assert(RC_LCOUNTER_BN + BN_COLUMN_LINES == RC_LCOUNTER_BNSEG, "column blocks of one reduction = the lines in front of the segmented forward's");
static_assert(36864 + (RC_LCOUNTER_BNSEG + BN_SEG_LINES) * RC_LINE_STRIDE * 4 <= 102400, "the segmented forward's lines end before the tree's");
static_assert(102400 + BN_TREE_LINES * RC_LINE_STRIDE * 4 == RC_ZERO_PAGE_BYTES, "the tree's lines are the end of the zero page");

// the tensors and scalars of one call; what a direction does not use stays zero
struct BnCall {
  const void *x, *y, *dy;                     // y: the forward's output as the backward reads it
  void* out;                                  // y of the forward, dx of the backward
  const int32_t* labels;
  const float *gamma, *beta;                  // backward: beta only where the activation mask is recomputed from x
  const float *mean_in, *rstd_in;             // statistics read (apply, backward)
  float *mean, *rstd, *mm, *mv;               // statistics written
  float eps, decay;
  float *dgamma, *dbeta;
  int act, accumulate, accumulate_dx;
};

// What every entry point refuses before it launches anything.  `tensors`: the ones the call reads or writes on every route.
static int bn_check_args(rcgan_ctx* ctx, const BnShape& s, const int32_t* labels, std::initializer_list<const void*> tensors) {
  RC_REQUIRE(ctx, s.nseg >= 1 && s.n >= 1 && s.rows_per_sample >= 1 && s.c >= 1, "bad shape: %d segments x %d samples x %d rows x %d channels",
             s.nseg, s.n, s.rows_per_sample, s.c);
  RC_REQUIRE(ctx, s.n_labels >= 1 && s.n_labels <= BN_MAX_LABELS_WIDE, "n_labels %d (1 .. %d)", s.n_labels, BN_MAX_LABELS_WIDE);
  RC_REQUIRE(ctx, labels != nullptr || s.n_labels == 1, "labels required for n_labels > 1");
  // (bn_plan.h: a segment's rows are an int in the kernels' arguments, the fused apply's chunk index has 32 bits)
  RC_REQUIRE(ctx, bn_index_ok(s), "%d x %ld rows x %d channels exceed the index types", s.nseg, s.rows(), s.c);
  for (const void* t : tensors) RC_REQUIRE(ctx, t != nullptr, "null tensor");
  return RCGAN_OK;
}

// ---- reduce: tree or column, statistics (MODE 0) or backward (MODE 1), nseg as the grid's last dimension ----
static BnFusedArgs bn_fused_args(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* ws) {
  BnFusedArgs a = {};
  a.rows = s.rows(); a.c = s.c; a.rows_per_group = p.rows_per_group; a.ngroups = p.workgroups;
  // (the kernels ask "nseg > 1": the tree is always told the count, the column kernel only by the segmented forward)
  a.nseg = (p.route == BN_TREE || s.op == BN_OP_STATS_SEG) ? s.nseg : 0;
  a.x = t.x; a.partial = ws + p.partial;
  if (p.route == BN_COLUMN) a.counter = ctx->line_counters() + (s.op == BN_OP_STATS_SEG ? RC_LCOUNTER_BNSEG : RC_LCOUNTER_BN) * RC_LINE_STRIDE;
  if (s.op != BN_OP_BWD) {
    a.eps = t.eps; a.mean = t.mean; a.rstd = t.rstd; a.mm = t.mm; a.mv = t.mv; a.decay = t.decay;
    return a;
  }
  a.y = t.y; a.dy = t.dy; a.mean_in = t.mean_in; a.rstd_in = t.rstd_in; a.act = t.act;
  a.n_labels = s.n_labels; a.groups_per_sample = p.groups_per_sample; a.labels = t.labels; a.n_samples = s.n;
  a.gamma = t.gamma; a.dgamma = t.dgamma; a.dbeta = t.dbeta; a.accumulate = t.accumulate;
  // mask from x needs a group's rows to belong to one sample (conditional grouping) or no labels at all
  a.beta = t.beta;
  a.PQ = ws + p.PQ;
  if (p.route == BN_COLUMN) a.nsub = p.nsub;
  return a;
}

template <int MODE>
static int launch_bn_tree(rcgan_ctx* ctx, int dtype, const BnFusedArgs& a, const BnPlan& p, int nseg, float* ws) {
  const size_t c = a.c, lds = p.lds;
  RC_REQUIRE(ctx, (size_t)nseg * (p.nclusters + 1) <= BN_TREE_LINES, "too many clusters (%d x %d)", nseg, p.nclusters);
  RC_REQUIRE(ctx, (size_t)p.ngroups * 2 * c * 4 < (1ull << 31) && (size_t)p.nclusters * 2 * c * 4 < (1ull << 31), "partials exceed a buffer descriptor");
  RC_REQUIRE(ctx, lds <= BN_TREE_MAX_LDS, "tree reduction needs %zu bytes of LDS", lds);
  BnTreeArgs ta;
  ta.f = a;
  ta.cpart = ws + p.cpart;
  ta.counters = ctx->tree_line_counters();
  ta.cs = p.cluster_size; ta.nclusters = p.nclusters;
  if (dtype == RCGAN_F32) {
    static size_t set = 0;
    if (lds > set) { RC_HIP(ctx, hipFuncSetAttribute((const void*)bn_tree_reduce_kernel<float, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); set = lds; }
    hipLaunchKernelGGL((bn_tree_reduce_kernel<float, MODE>), dim3(p.grid_x, p.grid_y), dim3(256), lds, ctx->stream, ta);
  } else if (dtype == RCGAN_H16) {
    static size_t set = 0;
    if (lds > set) { RC_HIP(ctx, hipFuncSetAttribute((const void*)bn_tree_reduce_kernel<bf16_t, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); set = lds; }
    hipLaunchKernelGGL((bn_tree_reduce_kernel<bf16_t, MODE>), dim3(p.grid_x, p.grid_y), dim3(256), lds, ctx->stream, ta);
  } else {
    RC_FAIL(ctx, RCGAN_EINVALID_ARG, "bad dtype %d", dtype);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

template <int MODE>
static int bn_launch_reduce(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* ws) {
  const BnFusedArgs a = bn_fused_args(ctx, s, p, t, ws);
  if (p.route == BN_TREE) return launch_bn_tree<MODE>(ctx, s.dtype, a, p, s.nseg, ws);
  RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL((bn_fused_reduce_kernel<T, MODE>), dim3(p.grid_x, p.grid_y, s.nseg), dim3(256), p.lds, ctx->stream, a));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// ---- partial + finish: vec or scalar partials per row group, then the statistics / the per-label sums; the wide backward's
// per-sample partials and class kernel ----
template <int MODE>
static int bn_launch_partial(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* partial) {
  const dim3 grid(p.grid_x, p.grid_y);
  const long rows = s.rows();
  if (p.route == BN_WIDE && p.partial_vec) {
    const float* bm = p.apply == BN_COLUMN ? t.beta : nullptr;        // the mask from x wherever the apply also takes it
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_sample_partial_kernel<T>, grid, dim3(256), 0, ctx->stream, s.rows_per_sample, s.c,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.labels, t.gamma, bm, t.mean_in, t.rstd_in,
                                                       t.act, partial));
  } else if (p.partial_vec) {
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL((bn_partial_vec_kernel<T, MODE>), grid, dim3(256), 0, ctx->stream, rows, s.c, p.rows_per_group,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.mean_in, t.rstd_in, t.act, partial));
  } else {
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL((bn_partial_kernel<T, MODE>), grid, dim3(256), 0, ctx->stream, rows, s.c, p.rows_per_group,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.mean_in, t.rstd_in, t.act, partial));
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

static int bn_launch_partial_finish(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* ws) {
  float* partial = ws + p.partial;
  const int c = s.c;
  if (int rc = s.op == BN_OP_BWD ? bn_launch_partial<1>(ctx, s, p, t, partial) : bn_launch_partial<0>(ctx, s, p, t, partial)) return rc;
  if (s.op != BN_OP_BWD)
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(cdiv(c, 256)), dim3(256), 0, ctx->stream, c, p.ngroups, s.rows(), (const float*)partial, t.eps,
                       t.mean, t.rstd, t.mm, t.mv, t.decay);
  else if (p.route == BN_WIDE)
    hipLaunchKernelGGL(bn_bwd_class_kernel, dim3(cdiv(c, 256), s.n_labels + 1), dim3(256), 0, ctx->stream, s.n, c, s.n_labels, s.rows(), t.labels,
                       t.gamma, (const float*)partial, t.mean_in, t.rstd_in, t.dgamma, t.dbeta, t.accumulate, ws + p.s12, ws + p.PQ);
  else
    hipLaunchKernelGGL(bn_bwd_combine_kernel, dim3(cdiv(c, 128)), dim3(128), 0, ctx->stream, c, p.ngroups, s.n_labels, t.labels, t.gamma,
                       (const float*)partial, t.dgamma, t.dbeta, ws + p.s12, t.accumulate);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// workspace check, then the reduction the plan names
static int bn_reduce(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, void* ws) {
  if (s.ws_bytes < p.need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", p.need, s.ws_bytes);
  if (p.route != BN_TREE && p.route != BN_COLUMN) return bn_launch_partial_finish(ctx, s, p, t, (float*)ws);
  return s.op == BN_OP_BWD ? bn_launch_reduce<1>(ctx, s, p, t, (float*)ws) : bn_launch_reduce<0>(ctx, s, p, t, (float*)ws);
}

// ---- forward apply: fused (nseg segments in one launch), vec with tables, or scalar ----
static int bn_launch_apply_fwd(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* ws) {
  const int rps = s.rows_per_sample, c = s.c;
  if (p.apply == BN_COLUMN) {
    const int seg_samples = s.op == BN_OP_APPLY ? 0 : s.n;            // samples per segment; 0: the call has no segments
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_apply_fused_kernel<T>, dim3(p.apply_grid, s.nseg), dim3(256), 0, ctx->stream, p.apply_items,
                                                       rps, c, (const T*)t.x, t.labels, t.gamma, t.beta, t.mean_in, t.rstd_in, t.act, (T*)t.out,
                                                       seg_samples));
  } else if (p.apply == BN_VEC) {
    float *A = ws + p.A, *B = ws + p.B;
    hipLaunchKernelGGL(bn_table_fwd_kernel, dim3(cdiv((long)s.n_labels * c, 256)), dim3(256), 0, ctx->stream, s.n_labels, c, t.gamma, t.beta,
                       t.mean_in, t.rstd_in, A, B);
    RC_LAUNCH_CHECK(ctx);
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_apply_vec_kernel<T>, dim3(p.apply_grid), dim3(256), 0, ctx->stream, p.apply_items, rps, c,
                                                       (const T*)t.x, t.labels, (const float*)A, (const float*)B, t.act, (T*)t.out));
  } else {
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_apply_fwd_kernel<T>, dim3(p.apply_grid), dim3(256), 0, ctx->stream, p.apply_items, rps, c,
                                                       (const T*)t.x, t.labels, t.gamma, t.beta, t.mean_in, t.rstd_in, t.act, (T*)t.out));
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// ---- backward apply: fused (dx constants PQ), vec with tables, or scalar (batch sums s12) ----
static int bn_launch_apply_bwd(rcgan_ctx* ctx, const BnShape& s, const BnPlan& p, const BnCall& t, float* ws) {
  const int rps = s.rows_per_sample, c = s.c;
  const long rows = s.rows();
  if (p.apply == BN_COLUMN) {
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_bwd_apply_fused_kernel<T>, dim3(p.apply_grid), dim3(256), 0, ctx->stream, p.apply_items, rps, c,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.labels, t.gamma, t.rstd_in,
                                                       (const float*)(ws + p.PQ), t.act, (T*)t.out, t.accumulate_dx, t.beta, t.mean_in));
  } else if (p.apply == BN_VEC) {
    float *A = ws + p.A, *PQ = ws + p.PQ;
    hipLaunchKernelGGL(bn_table_bwd_kernel, dim3(cdiv((long)s.n_labels * c, 256)), dim3(256), 0, ctx->stream, s.n_labels, c, rows, t.gamma, t.mean_in,
                       t.rstd_in, (const float*)(ws + p.s12), A, PQ);
    RC_LAUNCH_CHECK(ctx);
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_bwd_apply_vec_kernel<T>, dim3(p.apply_grid), dim3(256), 0, ctx->stream, p.apply_items, rps, c,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.labels, (const float*)A, (const float*)PQ,
                                                       t.act, (T*)t.out, t.accumulate_dx));
  } else {
    RC_DISPATCH_DTYPE(ctx, s.dtype, hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(p.apply_grid), dim3(256), 0, ctx->stream, p.apply_items, rows, rps, c,
                                                       (const T*)t.x, (const T*)t.y, (const T*)t.dy, t.labels, t.gamma, t.mean_in, t.rstd_in,
                                                       (const float*)(ws + p.s12), t.act, (T*)t.out, t.accumulate_dx));
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// The segmented calls' fallback: one segment at a time through the one-segment entry points, which choose their own route --
// statistics (rcgan_bn_fwd_segments) and, where the call has an output, the apply.
static int bn_each_segment(rcgan_ctx* ctx, bool with_stats, const BnShape& s, const BnCall& t, void* ws) {
  const long rows = s.rows();
  const size_t seg_bytes = (size_t)rows * s.c * dtype_size(s.dtype);
  for (int sg = 0; sg < s.nseg; ++sg) {
    const char* xs = (const char*)t.x + sg * seg_bytes;
    const size_t so = (size_t)sg * s.c;
    if (with_stats)
      if (int rc = rcgan_bn_stats(ctx, (int)rows, s.c, s.dtype, xs, t.eps, t.mean + so, t.rstd + so, nullptr, nullptr, 0.f, ws, s.ws_bytes)) return rc;
    if (!t.out) continue;
    if (int rc = rcgan_bn_apply_fwd(ctx, s.n, s.rows_per_sample, s.c, s.n_labels, s.dtype, xs, t.labels ? t.labels + (size_t)sg * s.n : nullptr, t.gamma,
                                    t.beta, t.mean_in + so, t.rstd_in + so, t.act, (char*)t.out + sg * seg_bytes, ws, s.ws_bytes))
      return rc;
  }
  return RCGAN_OK;
}

extern "C" {

size_t rcgan_bn_workspace_bytes(int rows, int c) {
  // stats: ngroups*2*c ; bwd: ngroups*2*c + 2*c, with ngroups <= max(rows/512, n) <= rows; the tree path adds its cluster
  // partials (<= one per group)
  long ng = (rows + 511) / 512 + 1;
  if (ng < 4096) ng = 4096;   // per-sample grouping (n <= 4096 samples)
  ng *= 2;
  return (size_t)(ng * 2 * (long)c + 4 * (long)c + 2 * MAX_LABELS * (long)c) * sizeof(float) + 256;
}

size_t rcgan_bn_workspace_bytes_labels(int rows, int c, int n_labels) {
  // the rule above with the per-label staging of the table paths ([2][n_labels][c]) sized for n_labels instead of MAX_LABELS
  const size_t base = rcgan_bn_workspace_bytes(rows, c);
  return n_labels > MAX_LABELS ? base + (size_t)2 * (n_labels - MAX_LABELS) * c * sizeof(float) : base;
}

int rcgan_bn_stats(rcgan_ctx* ctx, int rows, int c, int dtype, const void* x, float eps, float* mean, float* rstd,
                   float* mm, float* mv, float decay, void* ws, size_t ws_bytes) {
  const BnShape s = {BN_OP_STATS, 1, 1, rows, c, 1, false, dtype, ws_bytes};
  BnCall t = {};
  t.x = x; t.eps = eps; t.mean = mean; t.rstd = rstd; t.mm = mm; t.mv = mv; t.decay = decay;
  if (int rc = bn_check_args(ctx, s, nullptr, {x, mean, rstd})) return rc;
  const BnRoute route = bn_choose(s).route;
  // kept as it was: a call the tree takes must also hold what the column route would need (checked first)
  if (route == BN_TREE) {
    const size_t need = bn_plan(s, BN_COLUMN).need;
    if (ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
  }
  return bn_reduce(ctx, s, bn_plan(s, route), t, ws);
}

int rcgan_bn_apply_fwd(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype, const void* x,
                       const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd,
                       int act, void* y, void* ws, size_t ws_bytes) {
  const BnShape s = {BN_OP_APPLY, 1, n, rows_per_sample, c, n_labels, labels != nullptr, dtype, ws_bytes};
  BnCall t = {};
  t.x = x; t.out = y; t.labels = labels; t.gamma = gamma; t.beta = beta; t.mean_in = mean; t.rstd_in = rstd; t.act = act;
  if (int rc = bn_check_args(ctx, s, labels, {x, gamma, beta, mean, rstd, y})) return rc;
  // (no workspace check: bn_choose takes the table route only where ws_bytes holds the tables)
  return bn_launch_apply_fwd(ctx, s, bn_plan(s, bn_choose(s).route), t, (float*)ws);
}

// Forward batch norm of `nseg` independent segments of n_per_seg samples each (x = the segments back to back): every
// segment gets its own batch statistics, exactly as nseg separate calls would, in two launches for all of them.
// mean / rstd: [nseg][c] scratch outputs.
int rcgan_bn_fwd_segments(rcgan_ctx* ctx, int nseg, int n_per_seg, int rows_per_sample, int c, int n_labels, int dtype, const void* x,
                          const int32_t* labels, const float* gamma, const float* beta, float eps, int act,
                          float* mean, float* rstd, void* y, void* ws, size_t ws_bytes) {
  const BnShape s = {BN_OP_STATS_SEG, nseg, n_per_seg, rows_per_sample, c, n_labels, labels != nullptr, dtype, ws_bytes};
  BnCall t = {};
  t.x = x; t.out = y; t.labels = labels; t.gamma = gamma; t.beta = beta; t.act = act;
  t.eps = eps; t.mean = mean; t.rstd = rstd; t.mean_in = mean; t.rstd_in = rstd;
  if (int rc = bn_check_args(ctx, s, labels, {x, mean, rstd})) return rc;
  RC_REQUIRE(ctx, !y || (gamma && beta), "null gamma / beta");
  const BnChoice ch = bn_choose(s);
  if (ch.per_segment) return bn_each_segment(ctx, true, s, t, ws);
  const BnPlan p = bn_plan(s, ch.route);
  if (int rc = bn_reduce(ctx, s, p, t, ws)) return rc;
  if (!y) return RCGAN_OK;             // statistics only: the consumer normalises on load (rcgan_conv2d_fwd_bn)
  return bn_launch_apply_fwd(ctx, s, p, t, (float*)ws);
}

int rcgan_bn_apply_segments(rcgan_ctx* ctx, int nseg, int n_per_seg, int rows_per_sample, int c, int n_labels, int dtype, const void* x,
                            const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                            void* y, void* ws, size_t ws_bytes) {
  const BnShape s = {BN_OP_APPLY_SEG, nseg, n_per_seg, rows_per_sample, c, n_labels, labels != nullptr, dtype, ws_bytes};
  BnCall t = {};
  t.x = x; t.out = y; t.labels = labels; t.gamma = gamma; t.beta = beta; t.mean_in = mean; t.rstd_in = rstd; t.act = act;
  if (int rc = bn_check_args(ctx, s, labels, {x, gamma, beta, mean, rstd, y})) return rc;
  const BnChoice ch = bn_choose(s);
  if (ch.per_segment) return bn_each_segment(ctx, false, s, t, ws);
  return bn_launch_apply_fwd(ctx, s, bn_plan(s, ch.route), t, (float*)ws);
}

int rcgan_bn_bwd(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype, const void* x, const void* y,
                 const void* dy, const int32_t* labels, const float* gamma, const float* mean, const float* rstd, int act,
                 void* dx, int accumulate_dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes) {
  return rcgan_bn_bwd2(ctx, n, rows_per_sample, c, n_labels, dtype, x, y, dy, labels, gamma, nullptr, mean, rstd, act, dx, accumulate_dx,
                       dgamma, dbeta, accumulate, ws, ws_bytes);
}

int rcgan_bn_bwd2(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype, const void* x, const void* y,
                  const void* dy, const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd,
                  int act, void* dx, int accumulate_dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes) {
  const BnShape s = {BN_OP_BWD, 1, n, rows_per_sample, c, n_labels, labels != nullptr, dtype, ws_bytes};
  BnCall t = {};
  t.x = x; t.y = y; t.dy = dy; t.out = dx; t.labels = labels; t.gamma = gamma; t.mean_in = mean; t.rstd_in = rstd; t.act = act;
  t.dgamma = dgamma; t.dbeta = dbeta; t.accumulate = accumulate; t.accumulate_dx = accumulate_dx;
  // with beta, ReLU / leaky ReLU masks are recomputed from x on the fused paths (two instead of three tensor reads per pass)
  t.beta = (beta && (act == RCGAN_ACT_RELU || act == RCGAN_ACT_LRELU)) ? beta : nullptr;
  if (int rc = bn_check_args(ctx, s, labels, {x, dy, gamma, mean, rstd, dx, dgamma, dbeta})) return rc;
  const BnPlan p = bn_plan(s, bn_choose(s).route);
  RC_REQUIRE(ctx, y || act == RCGAN_ACT_NONE || (t.beta && p.apply == BN_COLUMN), "the activation's derivative needs y");
  if (int rc = bn_reduce(ctx, s, p, t, ws)) return rc;
  return bn_launch_apply_bwd(ctx, s, p, t, (float*)ws);
}

int rcgan_bn_infer(rcgan_ctx* ctx, int rows, int c, int dtype, const void* x, const float* gamma, const float* beta,
                   const float* mm, const float* mv, float eps, int act, void* y) {
  RC_REQUIRE(ctx, rows >= 1 && c >= 1, "bad shape: %d rows x %d channels", rows, c);
  RC_REQUIRE(ctx, x && gamma && beta && mm && mv && y, "null tensor");
  long total = (long)rows * c;
  RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(bn_infer_kernel<T>, dim3(bn_apply_grid(total)), dim3(256), 0, ctx->stream, total, c,
                                                   (const T*)x, gamma, beta, mm, mv, eps, act, (T*)y));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_bn_infer_bwd(rcgan_ctx* ctx, int rows, int c, int dtype, const void* y, const void* dy, const float* gamma,
                       const float* mv, float eps, int act, void* dx, int accumulate) {
  // (every activation's derivative is taken from the OUTPUT: leaky ReLU keeps the sign, so y > 0 <=> x > 0 as for ReLU)
  RC_REQUIRE(ctx, act >= RCGAN_ACT_NONE && act <= RCGAN_ACT_SIGMOID, "activation %d", act);
  RC_REQUIRE(ctx, rows >= 1 && c >= 1, "bad shape: %d rows x %d channels", rows, c);
  RC_REQUIRE(ctx, dy && gamma && mv && dx && (y || act == RCGAN_ACT_NONE), "null tensor");
  long total = (long)rows * c;
  RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(bn_infer_bwd_kernel<T>, dim3(bn_apply_grid(total)), dim3(256), 0, ctx->stream, total, c,
                                                   (const T*)y, (const T*)dy, gamma, mv, eps, act, (T*)dx, accumulate));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
