// Training the generated-label-accuracy classifier on the engine (classifier.py): the pieces of its step that the GAN steps never
// needed -- sparse softmax cross-entropy, the option-A shortcut and its adjoint as one launch each, tf.train.MomentumOptimizer, and the
// input pipeline (random translation + mirror) over a data set that lives on the device -- and, for the MNIST classifier
// (mnist_classifier.py), relu + 2x2 max pooling and dropout with their adjoints.  All plain vector loads and stores.
#include "common.h"
#include "rng.h"

// ---------------------------------------------------------------------------------------------------------
// sparse softmax cross-entropy: a wavefront per row, lanes over the columns (<= 1024 = 16 per lane, held in registers)
// ---------------------------------------------------------------------------------------------------------
#define XENT_MAX_COLS 1024
#define XENT_PER_LANE (XENT_MAX_COLS / 64)
#define XENT_MAX_WG 1024

__device__ __forceinline__ float xent_grad_scale(float gs_host, const float* gs_dev) { return gs_dev ? gs_host * gs_dev[0] : gs_host; }

// partials: [gridDim.x] loss sums, then [gridDim.x] correct counts.  Rows are dealt to the wavefronts round-robin, so every partial and
// the final sums are formed in an order that depends on the shape alone: the same bits run to run.
__global__ __launch_bounds__(256) void softmax_xent_kernel(int rows, int cols, const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                            float weight, float* loss_acc, float* n_correct_acc, float* __restrict__ dlogits,
                                                            float gs_host, const float* gs_dev, float* partials, unsigned* counter) {
  __shared__ float red_l[4], red_c[4], red[4];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_rows = 1.f / (float)rows;
  const float gw = dlogits ? weight * xent_grad_scale(gs_host, gs_dev) * inv_rows : 0.f;
  float lsum = 0.f, csum = 0.f;
  for (long r = (long)blockIdx.x * 4 + wave; r < rows; r += (long)gridDim.x * 4) {
    const float* x = logits + r * cols;
    float v[XENT_PER_LANE];
    float m = -INFINITY;
    int mi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < XENT_PER_LANE; ++q) {
      const int j = q * 64 + lane;
      v[q] = j < cols ? x[j] : -INFINITY;
      if (v[q] > m) { m = v[q]; mi = j; }           // strictly greater: the lowest index of this lane's maxima
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < XENT_PER_LANE; ++q) {
      v[q] = expf(v[q] - m);                       // (-inf - m -> 0 in the columns past the end)
      s += v[q];
    }
    s = wave_sum(s);
    const int lab = labels[r];
    const bool lab_ok = (unsigned)lab < (unsigned)cols;
    const float xl = lab_ok ? x[lab] : 0.f;
    if (lab_ok) lsum += (m + logf(s)) - xl;
    csum += (lab_ok && mi == lab) ? 1.f : 0.f;
    if (dlogits) {
      const float inv_s = 1.f / s;
      float* d = dlogits + r * cols;
#pragma unroll
      for (int q = 0; q < XENT_PER_LANE; ++q) {
        const int j = q * 64 + lane;
        if (j < cols) d[j] = gw * (v[q] * inv_s - (j == lab ? 1.f : 0.f));
      }
    }
  }
  // ---- the sums over rows: per-workgroup partials, finished in workgroup order by the last workgroup to arrive ----
  if (lane == 0) { red_l[wave] = lsum; red_c[wave] = csum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    partials[gridDim.x + blockIdx.x] = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    // release: the two stores above are visible to whoever reads the counter after this increment
    const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = prev == gridDim.x - 1u ? 1 : 0;
    if (is_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
  }
  __syncthreads();
  if (!is_last) return;
  float tl = 0.f, tc = 0.f;
  for (unsigned w = threadIdx.x; w < gridDim.x; w += 256) {
    tl += __hip_atomic_load(partials + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tc += __hip_atomic_load(partials + gridDim.x + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  tl = block_sum256(tl, red);
  tc = block_sum256(tc, red);
  if (threadIdx.x == 0) {
    if (loss_acc) *loss_acc += weight * (tl * inv_rows);
    if (n_correct_acc) *n_correct_acc += tc;
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward-corrected cross-entropy (Patrini et al. 2017) on noisy labels: L = -log((softmax(z) . C)[noisy]); same skeleton as above.
// ct[noisy][y] = C[y][noisy], so the lanes of a row read one contiguous row of ct.  With m = max z, s = sum exp(z - m), and over the
// SUPPORT { y : ct[noisy][y] > 0 }  m2 = max z, a = sum ct exp(z - m2)  (its largest term is ct at the arg-max: a > 0, no log 0):
//   loss row = (m + logf(s)) - (m2 + logf(a)),   post = ct exp(z - m2) / a,   dlogits = gw (exp(z - m) / s - post).
// C = I: m2 = z[label], a = 1, logf(a) = 0, post = onehot -- the arithmetic of softmax_xent_kernel, operation for operation.
// A row whose label is outside [0, cols) or whose ct row has no positive entry: no loss, zero gradient and posterior rows, recovered -1.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_xent_forward_kernel(int rows, int cols, const float* __restrict__ logits,
                                                                    const int32_t* __restrict__ labels, const float* __restrict__ ct, float weight,
                                                                    float* loss_acc, float* n_correct_acc, float* __restrict__ dlogits,
                                                                    float* __restrict__ posterior, int32_t* __restrict__ recovered, float gs_host,
                                                                    const float* gs_dev, float* partials, unsigned* counter) {
  __shared__ float red_l[4], red_c[4], red[4];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_rows = 1.f / (float)rows;
  const float gw = dlogits ? weight * xent_grad_scale(gs_host, gs_dev) * inv_rows : 0.f;
  float lsum = 0.f, csum = 0.f;
  for (long r = (long)blockIdx.x * 4 + wave; r < rows; r += (long)gridDim.x * 4) {
    const float* x = logits + r * cols;
    const int lab = labels[r];
    const bool lab_ok = (unsigned)lab < (unsigned)cols;
    const float* crow = ct + (size_t)(lab_ok ? lab : 0) * cols;
    float v[XENT_PER_LANE], u[XENT_PER_LANE];
    float m = -INFINITY, m2 = -INFINITY;
    int mi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < XENT_PER_LANE; ++q) {
      const int j = q * 64 + lane;
      v[q] = j < cols ? x[j] : -INFINITY;
      u[q] = (lab_ok && j < cols) ? crow[j] : 0.f;
      if (v[q] > m) { m = v[q]; mi = j; }           // strictly greater: the lowest index of this lane's maxima
      if (u[q] > 0.f && v[q] > m2) m2 = v[q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
      m2 = fmaxf(m2, __shfl_xor(m2, o, 64));
    }
    const bool valid = lab_ok && m2 > -INFINITY;     // (wave-uniform)
    float s = 0.f, a = 0.f;
#pragma unroll
    for (int q = 0; q < XENT_PER_LANE; ++q) {
      u[q] = (valid && u[q] > 0.f) ? u[q] * expf(v[q] - m2) : 0.f;
      a += u[q];
      v[q] = expf(v[q] - m);                       // (-inf - m -> 0 in the columns past the end)
      s += v[q];
    }
    s = wave_sum(s);
    a = wave_sum(a);
    if (valid) lsum += (m + logf(s)) - (m2 + logf(a));
    csum += (lab_ok && mi == lab) ? 1.f : 0.f;
    const float inv_s = 1.f / s, inv_a = valid ? 1.f / a : 0.f;
    float pm = -INFINITY;
    int pi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < XENT_PER_LANE; ++q) {
      const int j = q * 64 + lane;
      u[q] = __fmul_rn(u[q], inv_a);                 // the posterior, rounded here whatever the gradient's expression contracts to
      if (j < cols && u[q] > pm) { pm = u[q]; pi = j; }
    }
    if (recovered) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(pm, o, 64);
        const int oi = __shfl_xor(pi, o, 64);
        if (om > pm || (om == pm && oi < pi)) { pm = om; pi = oi; }
      }
      if (lane == 0) recovered[r] = valid ? pi : -1;
    }
    if (posterior) {
      float* p = posterior + r * cols;
#pragma unroll
      for (int q = 0; q < XENT_PER_LANE; ++q) {
        const int j = q * 64 + lane;
        if (j < cols) p[j] = u[q];
      }
    }
    if (dlogits) {
      float* d = dlogits + r * cols;
#pragma unroll
      for (int q = 0; q < XENT_PER_LANE; ++q) {
        const int j = q * 64 + lane;
        if (j < cols) d[j] = valid ? gw * (v[q] * inv_s - u[q]) : 0.f;
      }
    }
  }
  // ---- the sums over rows: per-workgroup partials, finished in workgroup order by the last workgroup to arrive ----
  if (lane == 0) { red_l[wave] = lsum; red_c[wave] = csum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    partials[gridDim.x + blockIdx.x] = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    // release: the two stores above are visible to whoever reads the counter after this increment
    const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = prev == gridDim.x - 1u ? 1 : 0;
    if (is_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
  }
  __syncthreads();
  if (!is_last) return;
  float tl = 0.f, tc = 0.f;
  for (unsigned w = threadIdx.x; w < gridDim.x; w += 256) {
    tl += __hip_atomic_load(partials + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tc += __hip_atomic_load(partials + gridDim.x + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  tl = block_sum256(tl, red);
  tc = block_sum256(tc, red);
  if (threadIdx.x == 0) {
    if (loss_acc) *loss_acc += weight * (tl * inv_rows);
    if (n_correct_acc) *n_correct_acc += tc;
  }
}

// ---------------------------------------------------------------------------------------------------------
// option-A shortcut: y[n][h/2][w/2][2c] = 2x2 mean of x[n][h][w][c] in channels [c/2, c/2 + c), zeros elsewhere.
// The mean is formed exactly as meanpool2_fwd_kernel / resample2_vec_kernel form it: (((x00 + x10) + x01) + x11) * 0.25.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void shortcut_a_fwd_kernel(int n, int h, int w, int c, const T* __restrict__ x, T* __restrict__ y) {
  const int oh = h >> 1, ow = w >> 1, co = 2 * c, before = c >> 1;
  const size_t total = (size_t)n * oh * ow * co;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % co) - before;
    float v = 0.f;
    if (ch >= 0 && ch < c) {
      size_t p = i / co;
      const int x2 = (int)(p % ow);
      p /= ow;
      const int y2 = (int)(p % oh), b = (int)(p / oh);
      const T* s = x + (((size_t)b * h + 2 * y2) * w + 2 * x2) * c + ch;
      v = (((Elem<T>::ld(s) + Elem<T>::ld(s + (size_t)w * c)) + Elem<T>::ld(s + c)) + Elem<T>::ld(s + (size_t)w * c + c)) * 0.25f;
    }
    Elem<T>::st(y + i, v);
  }
}

// fp32, c % 8 == 0: four channels per thread (the padding boundaries c/2 and c/2 + c then fall between the groups)
__global__ void shortcut_a_fwd_vec_kernel(int n, int h, int w, int c, const float* __restrict__ x, float* __restrict__ y) {
  const int oh = h >> 1, ow = w >> 1, cq = (2 * c) >> 2, before = c >> 1;
  const size_t total = (size_t)n * oh * ow * cq;
  const size_t rowpitch = (size_t)w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cq) * 4 - before;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ch >= 0 && ch < c) {
      size_t p = i / cq;
      const int x2 = (int)(p % ow);
      p /= ow;
      const int y2 = (int)(p % oh), b = (int)(p / oh);
      const float* s = x + (((size_t)b * h + 2 * y2) * w + 2 * x2) * c + ch;
      const float4 a0 = *(const float4*)s, a1 = *(const float4*)(s + rowpitch), a2 = *(const float4*)(s + c), a3 = *(const float4*)(s + rowpitch + c);
      o.x = (((a0.x + a1.x) + a2.x) + a3.x) * 0.25f;
      o.y = (((a0.y + a1.y) + a2.y) + a3.y) * 0.25f;
      o.z = (((a0.z + a1.z) + a2.z) + a3.z) * 0.25f;
      o.w = (((a0.w + a1.w) + a2.w) + a3.w) * 0.25f;
    }
    *(float4*)(y + i * 4) = o;
  }
}

// adjoint: dx[n][h][w][c] (=|+=) 0.25 * dy[n][h/2][w/2][c/2 + ch]
template <typename T>
__global__ void shortcut_a_bwd_kernel(int n, int h, int w, int c, const T* __restrict__ dy, T* __restrict__ dx, int accumulate) {
  const int oh = h >> 1, ow = w >> 1, co = 2 * c, before = c >> 1;
  const size_t total = (size_t)n * h * w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    size_t p = i / c;
    const int xx = (int)(p % w);
    p /= w;
    const int yy = (int)(p % h), b = (int)(p / h);
    float v = 0.25f * Elem<T>::ld(dy + (((size_t)b * oh + (yy >> 1)) * ow + (xx >> 1)) * co + before + ch);
    if (accumulate) v += Elem<T>::ld(dx + i);
    Elem<T>::st(dx + i, v);
  }
}

__global__ void shortcut_a_bwd_vec_kernel(int n, int h, int w, int c, const float* __restrict__ dy, float* __restrict__ dx, int accumulate) {
  const int oh = h >> 1, ow = w >> 1, co = 2 * c, before = c >> 1, cq = c >> 2;
  const size_t total = (size_t)n * h * w * cq;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cq) * 4;
    size_t p = i / cq;
    const int xx = (int)(p % w);
    p /= w;
    const int yy = (int)(p % h), b = (int)(p / h);
    const float4 g = *(const float4*)(dy + (((size_t)b * oh + (yy >> 1)) * ow + (xx >> 1)) * co + before + ch);
    float4 o = make_float4(0.25f * g.x, 0.25f * g.y, 0.25f * g.z, 0.25f * g.w);
    if (accumulate) {
      const float4 d = *(const float4*)(dx + i * 4);
      o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
    }
    *(float4*)(dx + i * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------
// tf.train.MomentumOptimizer on a flat fp32 range; the first decay_count elements carry L2 weight decay
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sgd_elem(float& w, float g, float& a, float lr, float momentum, float wd, int nesterov, float gs) {
  const float gp = gs * g + wd * w;
  a = momentum * a + gp;
  w -= nesterov ? lr * (gp + momentum * a) : lr * a;
}

__global__ void sgd_momentum_kernel(size_t count, size_t decay_count, float* __restrict__ w, const float* __restrict__ g, float* __restrict__ accum,
                                    const float* __restrict__ hyper, float momentum, float weight_decay, int nesterov, float grad_scale) {
  const float lr = hyper[0];
  const size_t n4 = ((((size_t)w | (size_t)g | (size_t)accum) & 15) == 0) ? count / 4 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 wv = ((float4*)w)[i], av = ((float4*)accum)[i];
    const float4 gv = ((const float4*)g)[i];
    const size_t e = i * 4;
    sgd_elem(wv.x, gv.x, av.x, lr, momentum, e + 0 < decay_count ? weight_decay : 0.f, nesterov, grad_scale);
    sgd_elem(wv.y, gv.y, av.y, lr, momentum, e + 1 < decay_count ? weight_decay : 0.f, nesterov, grad_scale);
    sgd_elem(wv.z, gv.z, av.z, lr, momentum, e + 2 < decay_count ? weight_decay : 0.f, nesterov, grad_scale);
    sgd_elem(wv.w, gv.w, av.w, lr, momentum, e + 3 < decay_count ? weight_decay : 0.f, nesterov, grad_scale);
    ((float4*)w)[i] = wv;
    ((float4*)accum)[i] = av;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    float wv = w[i], av = accum[i];
    sgd_elem(wv, g[i], av, lr, momentum, i < decay_count ? weight_decay : 0.f, nesterov, grad_scale);
    w[i] = wv;
    accum[i] = av;
  }
}

// ---------------------------------------------------------------------------------------------------------
// input pipeline: sample i = image index[i], translated by (dy, dx) with zeros shifted in, then mirrored left-right
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void augment_cifar_kernel(int n, int n_images, const uint8_t* __restrict__ images, const int32_t* __restrict__ labels_all,
                                     const int32_t* __restrict__ index, const int32_t* __restrict__ shift_flip, int pad, T* __restrict__ y,
                                     int32_t* __restrict__ labels_out) {
  const size_t total = (size_t)n * 3072;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % 3);
    const int px = (int)((i / 3) % 1024);
    const int b = (int)(i / 3072);
    const int src = index[b];
    const bool src_ok = (unsigned)src < (unsigned)n_images;
    const int dy = min(max(shift_flip[b * 3 + 0], -pad), pad), dx = min(max(shift_flip[b * 3 + 1], -pad), pad);
    const int yy = px >> 5, xx = px & 31;
    const int sy = yy - dy, sx = (shift_flip[b * 3 + 2] ? 31 - xx : xx) - dx;
    float v = 0.f;
    if (src_ok && (unsigned)sy < 32u && (unsigned)sx < 32u) v = (float)images[(size_t)src * 3072 + ch * 1024 + sy * 32 + sx];
    Elem<T>::st(y + i, v);
    if (ch == 0 && px == 0 && labels_out) labels_out[b] = (src_ok && labels_all) ? labels_all[src] : -1;
  }
}

// ---------------------------------------------------------------------------------------------------------
// the MNIST label classifier's two memory-bound operators (mnist_classifier.py): relu + 2x2 max pool, dropout.
// ClsVec<T, N>: N consecutive channels / elements as one access -- 16 bytes (float4, eight 16-bit values) on the vector routes,
// 8 bytes (four 16-bit values: one Philox quad) in dropout, one element on the scalar routes.
// ---------------------------------------------------------------------------------------------------------
template <typename T, int N> struct ClsVec;
template <typename T> struct ClsVec<T, 1> {
  static __device__ __forceinline__ void ld(const T* p, float* v) { v[0] = Elem<T>::ld(p); }
  static __device__ __forceinline__ void st(T* p, const float* v) { Elem<T>::st(p, v[0]); }
};
template <> struct ClsVec<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 a = *(const float4*)p;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct ClsVec<bf16_t, 4> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const uint2 a = *(const uint2*)p;
    v[0] = bf16_to_f32((bf16_t)(a.x & 0xffff)); v[1] = bf16_to_f32((bf16_t)(a.x >> 16));
    v[2] = bf16_to_f32((bf16_t)(a.y & 0xffff)); v[3] = bf16_to_f32((bf16_t)(a.y >> 16));
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    uint2 a;
    a.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
    a.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
    *(uint2*)p = a;
  }
};
template <> struct ClsVec<bf16_t, 8> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const uint4 a = *(const uint4*)p;
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = bf16_to_f32((bf16_t)(w[j] & 0xffff)); v[2 * j + 1] = bf16_to_f32((bf16_t)(w[j] >> 16)); }
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)f32_to_bf16(v[2 * j]) | ((uint32_t)f32_to_bf16(v[2 * j + 1]) << 16);
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

// y[n][h/2][w/2][c] = max(0, max of the 2x2 window).  A thread owns one output pixel x N channels (c % N == 0).
template <typename T, int N>
__global__ void relu_maxpool2_fwd_kernel(int n, int h, int w, int c, const T* __restrict__ x, T* __restrict__ y) {
  const int oh = h >> 1, ow = w >> 1, cv = c / N;
  const size_t total = (size_t)n * oh * ow * cv, rowpitch = (size_t)w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cv) * N;
    size_t p = i / cv;
    const int x2 = (int)(p % ow);
    p /= ow;
    const int y2 = (int)(p % oh);
    const size_t b = p / oh;
    const T* s = x + ((b * h + 2 * y2) * w + 2 * x2) * c + ch;
    float a[N], q[N];
    ClsVec<T, N>::ld(s, a);
    ClsVec<T, N>::ld(s + c, q);
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = q[j] > a[j] ? q[j] : a[j];
    ClsVec<T, N>::ld(s + rowpitch, q);
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = q[j] > a[j] ? q[j] : a[j];
    ClsVec<T, N>::ld(s + rowpitch + c, q);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      a[j] = q[j] > a[j] ? q[j] : a[j];
      a[j] = a[j] > 0.f ? a[j] : 0.f;
    }
    ClsVec<T, N>::st(y + i * N, a);
  }
}

// The same thread layout over the OUTPUT pixels: a thread recomputes the first maximum of its window and writes the window's four
// dx vectors itself -- no atomics, no pre-zeroing.
template <typename T, int N>
__global__ void relu_maxpool2_bwd_kernel(int n, int h, int w, int c, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                         int accumulate) {
  const int oh = h >> 1, ow = w >> 1, cv = c / N;
  const size_t total = (size_t)n * oh * ow * cv, rowpitch = (size_t)w * c;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cv) * N;
    size_t p = i / cv;
    const int x2 = (int)(p % ow);
    p /= ow;
    const int y2 = (int)(p % oh);
    const size_t b = p / oh;
    const size_t at = ((b * h + 2 * y2) * w + 2 * x2) * c + ch;
    const size_t off[4] = {0, (size_t)c, rowpitch, rowpitch + c};          // (0,0), (0,1), (1,0), (1,1)
    float m[N], q[N], g[N];
    int k[N];
    ClsVec<T, N>::ld(x + at, m);
#pragma unroll
    for (int j = 0; j < N; ++j) k[j] = 0;
#pragma unroll
    for (int t = 1; t < 4; ++t) {
      ClsVec<T, N>::ld(x + at + off[t], q);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (q[j] > m[j]) { m[j] = q[j]; k[j] = t; }                        // strictly greater: the first maximum keeps the gradient
    }
    ClsVec<T, N>::ld(dy + i * N, g);
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = m[j] > 0.f ? g[j] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float o[N];
      if (accumulate) {
        ClsVec<T, N>::ld(dx + at + off[t], o);
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] += k[j] == t ? g[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = k[j] == t ? g[j] : 0.f;
      }
      ClsVec<T, N>::st(dx + at + off[t], o);
    }
  }
}

// Dropout: a thread per Philox quad = four consecutive elements; element i reads word i & 3 of quad base + i / 4 on either route.
// vec: the bases are aligned for a 4-element access (16 bytes fp32, 8 bytes 16-bit, 4 mask bytes); the last, cut quad goes element by element.
template <typename T>
__global__ void dropout_fwd_kernel(size_t count, float keep_prob, float scale, uint64_t seed, const uint64_t* __restrict__ state,
                                   const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ mask, int vec) {
  const uint64_t base = state ? state[0] : 0;
  const size_t nquad = (count + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (size_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4(base + q, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) keep[j] = (float)(r[j] >> 8) * (1.0f / 16777216.0f) < keep_prob;
    const size_t e = q * 4;
    if (vec && e + 4 <= count) {
      float v[4];
      ClsVec<T, 4>::ld(x + e, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = keep[j] ? v[j] * scale : 0.f;
      ClsVec<T, 4>::st(y + e, v);
      *(uchar4*)(mask + e) = make_uchar4(keep[0], keep[1], keep[2], keep[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < count) {
          Elem<T>::st(y + e + j, keep[j] ? Elem<T>::ld(x + e + j) * scale : 0.f);
          mask[e + j] = keep[j] ? 1 : 0;
        }
    }
  }
}

__global__ void dropout_advance_kernel(uint64_t* state, uint64_t n) { state[0] += n; }

template <typename T>
__global__ void dropout_bwd_kernel(size_t count, float scale, const uint8_t* __restrict__ mask, const T* __restrict__ dy, T* __restrict__ dx,
                                   int accumulate, int vec) {
  const size_t nquad = (count + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    if (vec && e + 4 <= count) {
      const uchar4 mk = *(const uchar4*)(mask + e);
      const bool keep[4] = {mk.x != 0, mk.y != 0, mk.z != 0, mk.w != 0};
      float g[4], o[4];
      ClsVec<T, 4>::ld(dy + e, g);
      if (accumulate) ClsVec<T, 4>::ld(dx + e, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = keep[j] ? __fmul_rn(g[j], scale) : 0.f;          // rounded here: never contracted into the sum below
        o[j] = accumulate ? o[j] + v : v;
      }
      ClsVec<T, 4>::st(dx + e, o);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < count) {
          const float v = mask[e + j] ? __fmul_rn(Elem<T>::ld(dy + e + j), scale) : 0.f;
          Elem<T>::st(dx + e + j, accumulate ? Elem<T>::ld(dx + e + j) + v : v);
        }
    }
  }
}

static inline bool cls_aligned16(const void* a, const void* b) { return ((((size_t)a) | ((size_t)b)) & 15) == 0; }

static inline int cls_grid(size_t count) {
  size_t b = (count + 255) / 256;
  if (b > 8192) b = 8192;
  return b < 1 ? 1 : (int)b;
}

extern "C" {

size_t rcgan_softmax_xent_workspace_bytes(int rows) {
  const int nwg = rows < 4 * XENT_MAX_WG ? cdiv(rows > 0 ? rows : 1, 4) : XENT_MAX_WG;
  return (size_t)nwg * 2 * sizeof(float);
}

int rcgan_softmax_xent_fwd_bwd(rcgan_ctx* ctx, int rows, int cols, const float* logits, const int32_t* labels, float weight, float* loss_acc,
                               float* n_correct_acc, float* dlogits, void* ws, size_t ws_bytes) {
  RC_REQUIRE(ctx, rows >= 1 && logits && labels, "bad arguments (rows %d)", rows);
  if (cols < 2 || cols > XENT_MAX_COLS) RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "%d classes (2..%d)", cols, XENT_MAX_COLS);
  const size_t need = rcgan_softmax_xent_workspace_bytes(rows);
  if (!ws || ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
  const int nwg = (int)(need / (2 * sizeof(float)));
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(nwg), dim3(256), 0, ctx->stream, rows, cols, logits, labels, weight, loss_acc, n_correct_acc, dlogits,
                     ctx->gscale_host, ctx->gscale_dev, (float*)ws, ctx->counters() + RC_COUNTER_XENT);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_softmax_xent_forward_fwd_bwd(rcgan_ctx* ctx, int rows, int cols, const float* logits, const int32_t* labels, const float* ct, float weight,
                                       float* loss_acc, float* n_correct_acc, float* dlogits, float* posterior, int32_t* recovered, void* ws,
                                       size_t ws_bytes) {
  RC_REQUIRE(ctx, rows >= 1 && logits && labels && ct, "bad arguments (rows %d)", rows);
  if (cols < 2 || cols > XENT_MAX_COLS) RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "%d classes (2..%d)", cols, XENT_MAX_COLS);
  const size_t need = rcgan_softmax_xent_workspace_bytes(rows);
  if (!ws || ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
  const int nwg = (int)(need / (2 * sizeof(float)));
  // (the counter of softmax_xent_kernel: launches of one stream, and each leaves it at zero)
  hipLaunchKernelGGL(softmax_xent_forward_kernel, dim3(nwg), dim3(256), 0, ctx->stream, rows, cols, logits, labels, ct, weight, loss_acc,
                     n_correct_acc, dlogits, posterior, recovered, ctx->gscale_host, ctx->gscale_dev, (float*)ws, ctx->counters() + RC_COUNTER_XENT);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_shortcut_a_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y) {
  RC_REQUIRE(ctx, n >= 1 && c >= 2 && h >= 2 && w >= 2 && x && y, "bad arguments");
  RC_REQUIRE(ctx, h % 2 == 0 && w % 2 == 0 && c % 2 == 0, "odd shape %dx%dx%d", h, w, c);
  const size_t cnt = (size_t)n * (h / 2) * (w / 2) * 2 * c;
  if (dtype == RCGAN_F32 && c % 8 == 0 && cls_aligned16(x, y)) {
    hipLaunchKernelGGL(shortcut_a_fwd_vec_kernel, dim3(cls_grid(cnt / 4)), dim3(256), 0, ctx->stream, n, h, w, c, (const float*)x, (float*)y);
  } else {
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(shortcut_a_fwd_kernel<T>, dim3(cls_grid(cnt)), dim3(256), 0, ctx->stream, n, h, w, c, (const T*)x, (T*)y));
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_shortcut_a_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* dy, void* dx, int accumulate) {
  RC_REQUIRE(ctx, n >= 1 && c >= 2 && h >= 2 && w >= 2 && dy && dx, "bad arguments");
  RC_REQUIRE(ctx, h % 2 == 0 && w % 2 == 0 && c % 2 == 0, "odd shape %dx%dx%d", h, w, c);
  const size_t cnt = (size_t)n * h * w * c;
  if (dtype == RCGAN_F32 && c % 8 == 0 && cls_aligned16(dy, dx)) {
    hipLaunchKernelGGL(shortcut_a_bwd_vec_kernel, dim3(cls_grid(cnt / 4)), dim3(256), 0, ctx->stream, n, h, w, c, (const float*)dy, (float*)dx, accumulate);
  } else {
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(shortcut_a_bwd_kernel<T>, dim3(cls_grid(cnt)), dim3(256), 0, ctx->stream, n, h, w, c, (const T*)dy, (T*)dx, accumulate));
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_sgd_momentum(rcgan_ctx* ctx, size_t count, size_t decay_count, float* w, const float* g, float* accum, const float* hyper, float momentum,
                       float weight_decay, int nesterov, float grad_scale) {
  RC_REQUIRE(ctx, w && g && accum && hyper, "null pointer");
  RC_REQUIRE(ctx, decay_count <= count, "decay_count %zu > count %zu", decay_count, count);
  if (count == 0) return RCGAN_OK;
  hipLaunchKernelGGL(sgd_momentum_kernel, dim3(cls_grid((count + 3) / 4)), dim3(256), 0, ctx->stream, count, decay_count, w, g, accum, hyper, momentum,
                     weight_decay, nesterov ? 1 : 0, grad_scale);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_augment_cifar(rcgan_ctx* ctx, int n, int n_images, const uint8_t* images_chw_u8, const int32_t* labels_all, const int32_t* index,
                        const int32_t* shift_flip, int pad, int dtype, void* y_nhwc, int32_t* labels_out) {
  RC_REQUIRE(ctx, n >= 1 && n_images >= 1 && images_chw_u8 && index && shift_flip && y_nhwc, "bad arguments");
  RC_REQUIRE(ctx, pad >= 0 && pad < 32, "pad %d", pad);
  RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(augment_cifar_kernel<T>, dim3(cls_grid((size_t)n * 3072)), dim3(256), 0, ctx->stream, n, n_images,
                                                   images_chw_u8, labels_all, index, shift_flip, pad, (T*)y_nhwc, labels_out));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// 16-byte accesses along the channel axis: c a multiple of 4 (fp32) / 8 (16-bit) keeps every pixel's vectors aligned when the bases are
static inline bool cls_pool_vec(int dtype, int c, const void* a, const void* b, const void* d) {
  return c % (dtype == RCGAN_F32 ? 4 : 8) == 0 && ((((size_t)a) | ((size_t)b) | ((size_t)d)) & 15) == 0;
}

int rcgan_relu_maxpool2_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y) {
  RC_REQUIRE(ctx, n >= 1 && h >= 1 && w >= 1 && c >= 1, "bad shape %dx%dx%dx%d", n, h, w, c);
  RC_REQUIRE(ctx, h % 2 == 0 && w % 2 == 0, "odd spatial size %dx%d", h, w);
  RC_REQUIRE(ctx, x && y, "null pointer");
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  const size_t cnt = (size_t)n * (h / 2) * (w / 2) * c;
  if (!cls_pool_vec(dtype, c, x, y, nullptr)) {
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL((relu_maxpool2_fwd_kernel<T, 1>), dim3(cls_grid(cnt)), dim3(256), 0, ctx->stream, n, h, w, c, (const T*)x, (T*)y));
  } else if (dtype == RCGAN_F32) {
    hipLaunchKernelGGL((relu_maxpool2_fwd_kernel<float, 4>), dim3(cls_grid(cnt / 4)), dim3(256), 0, ctx->stream, n, h, w, c, (const float*)x, (float*)y);
  } else {
    hipLaunchKernelGGL((relu_maxpool2_fwd_kernel<bf16_t, 8>), dim3(cls_grid(cnt / 8)), dim3(256), 0, ctx->stream, n, h, w, c, (const bf16_t*)x, (bf16_t*)y);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_relu_maxpool2_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, const void* dy, void* dx, int accumulate) {
  RC_REQUIRE(ctx, n >= 1 && h >= 1 && w >= 1 && c >= 1, "bad shape %dx%dx%dx%d", n, h, w, c);
  RC_REQUIRE(ctx, h % 2 == 0 && w % 2 == 0, "odd spatial size %dx%d", h, w);
  RC_REQUIRE(ctx, x && dy && dx, "null pointer");
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  const size_t cnt = (size_t)n * (h / 2) * (w / 2) * c;
  const int acc = accumulate ? 1 : 0;
  if (!cls_pool_vec(dtype, c, x, dy, dx)) {
    RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL((relu_maxpool2_bwd_kernel<T, 1>), dim3(cls_grid(cnt)), dim3(256), 0, ctx->stream, n, h, w, c, (const T*)x, (const T*)dy, (T*)dx, acc));
  } else if (dtype == RCGAN_F32) {
    hipLaunchKernelGGL((relu_maxpool2_bwd_kernel<float, 4>), dim3(cls_grid(cnt / 4)), dim3(256), 0, ctx->stream, n, h, w, c, (const float*)x, (const float*)dy, (float*)dx, acc);
  } else {
    hipLaunchKernelGGL((relu_maxpool2_bwd_kernel<bf16_t, 8>), dim3(cls_grid(cnt / 8)), dim3(256), 0, ctx->stream, n, h, w, c, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, acc);
  }
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

// a 4-element access of every tensor of a dropout call: 16 bytes fp32, 8 bytes 16-bit, 4 mask bytes
static inline int cls_dropout_vec(int dtype, const void* a, const void* b, const void* mask) {
  const size_t m = dtype == RCGAN_F32 ? 15 : 7;
  return ((((size_t)a) | ((size_t)b)) & m) == 0 && (((size_t)mask) & 3) == 0;
}

int rcgan_dropout_fwd(rcgan_ctx* ctx, size_t count, int dtype, float keep_prob, uint64_t seed, void* state, const void* x, void* y, uint8_t* mask) {
  RC_REQUIRE(ctx, count >= 1, "empty tensor");
  RC_REQUIRE(ctx, x && y && mask, "null pointer");
  RC_REQUIRE(ctx, keep_prob > 0.f && keep_prob <= 1.f, "keep_prob %g outside (0, 1]", keep_prob);      // (a NaN fails both)
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  const float scale = 1.0f / keep_prob;
  const size_t nquad = (count + 3) / 4;
  RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(dropout_fwd_kernel<T>, dim3(cls_grid(nquad)), dim3(256), 0, ctx->stream, count, keep_prob, scale, seed,
                                                   (const uint64_t*)state, (const T*)x, (T*)y, mask, cls_dropout_vec(dtype, x, y, mask)));
  RC_LAUNCH_CHECK(ctx);
  if (state) {
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, ctx->stream, (uint64_t*)state, (uint64_t)nquad);
    RC_LAUNCH_CHECK(ctx);
  }
  return RCGAN_OK;
}

int rcgan_dropout_bwd(rcgan_ctx* ctx, size_t count, int dtype, float keep_prob, const uint8_t* mask, const void* dy, void* dx, int accumulate) {
  RC_REQUIRE(ctx, count >= 1, "empty tensor");
  RC_REQUIRE(ctx, mask && dy && dx, "null pointer");
  RC_REQUIRE(ctx, keep_prob > 0.f && keep_prob <= 1.f, "keep_prob %g outside (0, 1]", keep_prob);
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  const float scale = 1.0f / keep_prob;
  RC_DISPATCH_DTYPE(ctx, dtype, hipLaunchKernelGGL(dropout_bwd_kernel<T>, dim3(cls_grid((count + 3) / 4)), dim3(256), 0, ctx->stream, count, scale, mask,
                                                   (const T*)dy, (T*)dx, accumulate ? 1 : 0, cls_dropout_vec(dtype, dy, dx, mask)));
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
