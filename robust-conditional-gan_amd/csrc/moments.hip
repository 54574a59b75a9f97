// Per-class first and second moments of a feature stream (frechet.py): count[K], sum[K][d] and the full matrix sum x x^T [K][d][d],
// accumulated in fp64 from fp32 features, one launch per batch.  A product of two fp32 values is exact in fp64, so the only error is
// the order of the additions -- and that order depends on the shape alone: every entry of the state has ONE owner thread, which adds
// the rows of its class in row order and then adds that sum to the state (no floating-point atomics, the same bits run to run).
#include "common.h"

#define MOM_TILE 16                 // a workgroup owns a 16 x 16 tile of one class's matrix: one entry per thread
#define MOM_CHUNK 256               // rows whose labels are scanned at a time (one per thread)
#define MOM_MAX_D 256
#define MOM_MAX_CLASSES 1024

// grid = (tiles of the d x d matrix, classes).  Every workgroup scans the whole label vector (n is a few thousand at most: 4 bytes a
// row), keeps the rows of its class as an ordered list in LDS, and walks that list.  Column tile 0 also owns the class's sums, tile
// (0, 0) its count, and tile (0, 0) of class 0 the counter of rejected rows (labels outside [0, K): they match no workgroup's class,
// so they are written nowhere).
__global__ __launch_bounds__(256) void class_moments_kernel(int n, int d, int n_classes, const float* __restrict__ feat,
                                                             const int32_t* __restrict__ labels, double* __restrict__ state) {
  __shared__ int list[MOM_CHUNK];
  __shared__ int wave_cnt[4];
  __shared__ int rejected;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (d + MOM_TILE - 1) / MOM_TILE;
  const int ti = blockIdx.x / nt, tj = blockIdx.x % nt, k = blockIdx.y;
  const int i = ti * MOM_TILE + (tid >> 4), j = tj * MOM_TILE + (tid & 15);
  const bool own_entry = i < d && j < d;
  const bool own_sum = tj == 0 && (tid & 15) == 0 && i < d;
  const bool own_rejects = blockIdx.x == 0 && k == 0;
  if (tid == 0) rejected = 0;
  __syncthreads();
  double acc = 0.0, s = 0.0;
  long cnt = 0;
  for (long r0 = 0; r0 < n; r0 += MOM_CHUNK) {
    const long r = r0 + tid;
    const bool in = r < n;
    const int lab = in ? (labels ? labels[r] : 0) : -1;
    const bool match = in && lab == k;
    if (own_rejects && in && (unsigned)lab >= (unsigned)n_classes) atomicAdd(&rejected, 1);      // (an integer count in LDS)
    const unsigned long long b = __ballot(match);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    const int m = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
    if (match) list[off + __popcll(b & ((1ull << lane) - 1ull))] = (int)r;                     // ordered: rows stay in row order
    __syncthreads();
    if (own_entry) {
      int q = 0;
      for (; q + 4 <= m; q += 4) {            // four rows' loads in flight; the additions stay in row order
        const float* x0 = feat + (size_t)list[q] * d;
        const float* x1 = feat + (size_t)list[q + 1] * d;
        const float* x2 = feat + (size_t)list[q + 2] * d;
        const float* x3 = feat + (size_t)list[q + 3] * d;
        const float a0 = x0[i], b0 = x0[j], a1 = x1[i], b1 = x1[j], a2 = x2[i], b2 = x2[j], a3 = x3[i], b3 = x3[j];
        acc = fma((double)a0, (double)b0, acc);
        acc = fma((double)a1, (double)b1, acc);
        acc = fma((double)a2, (double)b2, acc);
        acc = fma((double)a3, (double)b3, acc);
        if (own_sum) s = (((s + (double)a0) + (double)a1) + (double)a2) + (double)a3;
      }
      for (; q < m; ++q) {
        const float* x = feat + (size_t)list[q] * d;
        const float a = x[i];
        acc = fma((double)a, (double)x[j], acc);
        if (own_sum) s += (double)a;
      }
    }
    cnt += m;
    __syncthreads();                          // the list and the counts are rewritten by the next chunk
  }
  const size_t K = (size_t)n_classes, D = (size_t)d;
  double* sum = state + K;
  double* sumsq = sum + K * D;
  if (own_entry) sumsq[((size_t)k * D + i) * D + j] += acc;
  if (own_sum) sum[(size_t)k * D + i] += s;
  if (blockIdx.x == 0 && tid == 0) {
    state[k] += (double)cnt;
    if (own_rejects) sumsq[K * D * D] += (double)rejected;
  }
}

extern "C" {

size_t rcgan_class_moments_bytes(int d, int n_classes) {
  if (d < 1 || d > MOM_MAX_D || n_classes < 1 || n_classes > MOM_MAX_CLASSES) return 0;
  const size_t K = (size_t)n_classes, D = (size_t)d;
  return (K + K * D + K * D * D + 1) * sizeof(double);
}

int rcgan_class_moments_accum(rcgan_ctx* ctx, int n, int d, int n_classes, const float* feat, const int32_t* labels, void* state) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool ok = n >= 1 && d >= 1 && d <= MOM_MAX_D && n_classes >= 1 && n_classes <= MOM_MAX_CLASSES && (labels || n_classes == 1) && feat &&
                  state && ((uintptr_t)state & 7) == 0 && ((uintptr_t)feat & 3) == 0 && ((uintptr_t)labels & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d (>= 1), d %d (1..%d), n_classes %d (1..%d), labels %s (NULL only with one class), feat / state %s", n, d, MOM_MAX_D,
             n_classes, MOM_MAX_CLASSES, labels ? "given" : "NULL", feat && state ? "given" : "NULL");
  const int nt = cdiv(d, MOM_TILE);
  hipLaunchKernelGGL(class_moments_kernel, dim3(nt * nt, n_classes), dim3(256), 0, ctx->stream, n, d, n_classes, feat, labels, (double*)state);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
