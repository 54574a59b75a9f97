// Row sums of the cubic polynomial kernel k(x, y) = (gamma <x, y> + coef0)^3 between fp32 feature rows (kid.py: the unbiased MMD^2
// "kernel distance"), without the n x m kernel matrix.  Rows are grouped into contiguous segments as in knn.hip: segment s of the
// queries only ever meets segment s of the references.
//
// Unlike a ball query's threshold comparison, a kernel SUM loses nothing to the inner-product form, so the inner products run on the
// matrix cores: v_mfma_f32_32x32x2_f32, exact fp32 (a chain of fmaf), |dot_c - dot| <= g_d sum_i |q_i r_i| with g_d = d u / (1 - d u),
// u = 2^-24, whatever the order.  Everything after the inner product is fp64: t = gamma * (double)dot_c + coef0, t * t * t, the sum.
// No floating-point atomics: the order in which a row's terms are added is fixed by the launch geometry (below), the same bits on
// every run.
//
// grid = (tiles of 64 query rows, segments), 512 threads.  The references are the M side of the MFMA and the queries the N side, so a
// lane's 16 accumulator entries are 16 reference rows of ONE query (column lane % 32) and the epilogue leaves one fp64 partial per
// lane.  Reference rows are staged through LDS in tiles of 128, double-buffered (the next tile's global loads are in flight while
// this one is multiplied, one barrier per tile); wavefront w takes reference rows 32 (w / 2) .. + 31 of the tile against queries
// 32 (w % 2) .. + 31.  A dot product does not care in which order the features are paired: of a chunk of 64 features the lower
// half-wave (k = 0 of every MFMA) takes features 0..31 and the upper (k = 1) features 32..63, on both operands, so a lane reads its
// 32 reference features as eight 16-byte LDS reads (row stride 68 floats: conflict-free) and keeps its 32 query features in
// registers.  Feature tails are staged as zeros, which add exactly nothing; reference rows past the segment's end and the excluded
// row are masked in the epilogue (a zero row would add coef0^3).  d > 64 walks the features in chunks of 64 with the accumulator kept
// and re-reads the query's chunk from global memory at every step (its loop waits for that load together with the next tile's; the
// d <= 64 instantiation, the evaluator's shape, loads the query once and multiplies with the next tile's loads in flight).
// 120 VGPRs (112 for d > 64), no scratch, 68 KiB of LDS: two workgroups per CU, so that one's epilogue (fp64, vector units) and
// barrier run under the other's MFMAs.
//
// A query's sum: per lane, tiles in ascending order and within a tile accumulator entries 0..15; then the 8 partials of the query
// (4 row blocks x 2 half-waves) are added through LDS in the order row block 0 lower, 0 upper, 1 lower, ... 3 upper.
#include "seg_rows.h"

#define KS_QT 64                     // query rows per workgroup: two MFMA column blocks of 32
#define KS_WAVES 8
#define KS_THREADS (64 * KS_WAVES)
#define KS_RB 32                     // reference rows per wavefront and tile: the MFMA's M
#define KS_TR (KS_RB * KS_WAVES / 2) // reference rows per staged tile: 128
#define KS_DC 64                     // features per chunk: a run of 32 per half-wave
#define KS_LD (KS_DC + 4)            // LDS row stride (floats): 16 lanes of a 16-byte read land on 16 different bank quads
#define KS_TILE (KS_TR * KS_LD)      // floats per LDS buffer

typedef __attribute__((ext_vector_type(16))) float ks_f32x16_t;

// ONE: d <= 64, the queries' features are loaded once, before the loop -- the loop's only global loads are then the next tile's, and
// nothing in it waits for them before the tile is multiplied.
template <bool ONE>
__global__ __launch_bounds__(KS_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void ksum_kernel(int nq, int nr, int d, int vec_q, int vec_r, const float* __restrict__ q,
                                                          const int32_t* __restrict__ q_off, const float* __restrict__ r,
                                                          const int32_t* __restrict__ r_off, double gamma, double coef0, int exclude,
                                                          double* __restrict__ rowsum) {
  __shared__ __attribute__((aligned(16))) float smem[2 * KS_TILE];           // two staged tiles; afterwards the merge area
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, seg = blockIdx.y;
  const int col = lane & 31, half = lane >> 5, qb = wave & 1, rb = wave >> 1;
  int qs, qe, rs, re;
  knn_segment(q_off, seg, nq, &qs, &qe);
  knn_segment(r_off, seg, nr, &rs, &re);
  const long q0 = (long)qs + (long)blockIdx.x * KS_QT;
  if (q0 >= qe) return;                                   // (the whole workgroup: no barrier has been met)
  const long qrow = q0 + qb * 32 + col;
  const bool q_ok = qrow < qe;
  const int nchunks = ONE ? 1 : (d + KS_DC - 1) / KS_DC;
  const int m = re - rs;
  const int ntiles = (m + KS_TR - 1) / KS_TR;
  const int nsteps = ntiles * nchunks;                    // step = (tile, chunk), chunk fastest

  float qreg[KS_DC / 2];
  auto load_q = [&](int c) {
#pragma unroll
    for (int i = 0; i < KS_DC / 2; i += 4) {
      const float4 v = knn_load4(q, (size_t)qrow, d, c * KS_DC + half * 32 + i, q_ok, vec_q != 0);
      qreg[i] = v.x; qreg[i + 1] = v.y; qreg[i + 2] = v.z; qreg[i + 3] = v.w;
    }
  };
  // staging: 2048 float4 per tile, four per thread
  float4 pf[4];
  auto fetch = [&](int step) {
    const int t = step / nchunks, c = step - t * nchunks;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = tid + KS_THREADS * u, row = f >> 4, c4 = (f & 15) * 4;
      const unsigned j = (unsigned)rs + (unsigned)t * KS_TR + row;        // (below 2^31 + 128: no wrap)
      pf[u] = knn_load4(r, (size_t)j, d, c * KS_DC + c4, j < (unsigned)re, vec_r != 0);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = tid + KS_THREADS * u, row = f >> 4, c4 = (f & 15) * 4;
      *(float4*)&smem[buf * KS_TILE + row * KS_LD + c4] = pf[u];
    }
  };

  if (nsteps == 0) {                                      // an empty reference segment gives 0.0 (the whole workgroup leaves)
    if (tid < KS_QT && q0 + tid < qe) rowsum[q0 + tid] = 0.0;
    return;
  }
  double sum = 0.0;
  ks_f32x16_t acc;
  if (ONE) load_q(0);
  fetch(0);
  stash(0);                                               // (waits for every load so far: the loop starts with none in flight)
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    const int t = step / nchunks, c = step - t * nchunks;
    const int nvalid = min(KS_TR, m - t * KS_TR);          // rows of this tile that exist
    const bool busy = rb * KS_RB < nvalid;                 // (uniform per wavefront: the MFMAs run with every lane on)
    if (!ONE && busy) load_q(c);                           // (requested BEFORE the next tile, so that waiting for it leaves that in flight)
    if (step + 1 < nsteps) fetch(step + 1);
    if (busy) {
      if (c == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      }
      const float* arow = &smem[buf * KS_TILE + (rb * KS_RB + col) * KS_LD + half * 32];
#pragma unroll
      for (int i = 0; i < KS_DC / 2; i += 4) {
        const float4 v = *(const float4*)&arow[i];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, qreg[i], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, qreg[i + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, qreg[i + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, qreg[i + 3], acc, 0, 0, 0);
      }
      if (c == nchunks - 1) {
        // the tile row that is this lane's own query (exclude_same_row), if it is in this tile; else no row
        const long own = qrow - ((long)rs + (long)t * KS_TR);
        const int skip = exclude && own >= 0 && own < KS_TR ? (int)own : -1;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = rb * KS_RB + (e & 3) + 8 * (e >> 2) + 4 * half;       // the MFMA's C/D map: the reference row of entry e
          const double v = fma(gamma, (double)acc[e], coef0);
          const double k3 = v * v * v;
          sum += row < nvalid && row != skip ? k3 : 0.0;   // (a row past the segment's end is zeros, not a reference; + 0.0 is exact)
        }
      }
    }
    if (step + 1 < nsteps) stash(buf ^ 1);
    __syncthreads();
  }

  // merge the 8 partials of every query in a fixed order (the last barrier above freed the tiles)
  double* md = (double*)smem;
  md[wave * 64 + lane] = sum;
  __syncthreads();
  if (tid < KS_QT && q0 + tid < qe) {
    const int b = tid >> 5, cc = tid & 31;
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < KS_WAVES / 2; ++w) {
      s += md[(w * 2 + b) * 64 + cc];
      s += md[(w * 2 + b) * 64 + 32 + cc];
    }
    rowsum[q0 + tid] = s;
  }
}

extern "C" {

int rcgan_poly3_rowsum(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const float* q, const int32_t* q_off, const float* r,
                       const int32_t* r_off, double gamma, double coef0, int exclude_same_row, double* rowsum) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool finite = gamma - gamma == 0.0 && coef0 - coef0 == 0.0;
  const bool ok = nq >= 1 && nr >= 1 && d >= 1 && d <= KNN_MAX_D && n_seg >= 1 && n_seg <= KNN_MAX_SEG && q && q_off && r && r_off && rowsum &&
                  finite && ((uintptr_t)q & 3) == 0 && ((uintptr_t)r & 3) == 0 && ((uintptr_t)q_off & 3) == 0 && ((uintptr_t)r_off & 3) == 0 &&
                  ((uintptr_t)rowsum & 7) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "nq %d, nr %d (>= 1), d %d (1..%d), n_seg %d (1..%d), gamma %g, coef0 %g (finite), q / q_off / r / r_off / rowsum %s", nq, nr,
             d, KNN_MAX_D, n_seg, KNN_MAX_SEG, gamma, coef0, q && q_off && r && r_off && rowsum ? "given" : "NULL");
  const dim3 grid(cdiv(nq, KS_QT), n_seg), block(KS_THREADS);
  if (d <= KS_DC)
    hipLaunchKernelGGL(ksum_kernel<true>, grid, block, 0, ctx->stream, nq, nr, d, knn_vec(q, d), knn_vec(r, d), q, q_off, r, r_off, gamma, coef0,
                       exclude_same_row != 0 ? 1 : 0, rowsum);
  else
    hipLaunchKernelGGL(ksum_kernel<false>, grid, block, 0, ctx->stream, nq, nr, d, knn_vec(q, d), knn_vec(r, d), q, q_off, r, r_off, gamma, coef0,
                       exclude_same_row != 0 ? 1 : 0, rowsum);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
