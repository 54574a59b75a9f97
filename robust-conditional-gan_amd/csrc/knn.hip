// k-nearest-neighbour radii and ball queries on fp32 feature rows (manifold.py: precision / recall / density / coverage), without the
// n x m distance matrix.  Rows are grouped into contiguous segments (one for the pooled metric, one per class); segment s of the
// queries only ever meets segment s of the references.
//
// A squared distance is the fp32 sum of (a_i - b_i)^2 over ascending i, every term non-negative: |computed - exact| <= (d + 3) 2^-24 exact.
// It is NOT |a|^2 + |b|^2 - 2 a.b -- the results are thresholds (dist <= radius^2) and the expanded form loses them to cancellation --
// so there is nothing here for the matrix cores.  The k-th smallest of a multiset, an integer count and a minimum do not depend on the
// order in which partial results are merged: no floating-point atomics, the same bits on every run.
//
// grid = (tiles of 64 query rows, segments), 512 threads.  One lane owns one query row (64 of its features in registers at a time); the
// 8 wavefronts of a workgroup own the SAME 64 queries and split every staged tile of 64 reference rows between them (8 rows each),
// then merge their sorted lists / counts / minima through LDS.  Reference rows are staged through LDS, double-buffered (the next
// tile's global loads are in flight while this one is computed); every lane reads them at the same address (a broadcast).  d > 64
// walks the features in chunks of 64 with the 8 partial sums kept in registers.
#include "seg_rows.h"

#define KNN_MAX_K 16
#define KNN_QT 64                    // query rows per workgroup: one per lane
#define KNN_WAVES 8
#define KNN_THREADS (64 * KNN_WAVES)
#define KNN_TR 64                    // reference rows per staged tile
#define KNN_RW (KNN_TR / KNN_WAVES)  // ... of which a wavefront takes this many
#define KNN_DC 64                    // features per chunk
#define KNN_TILE (KNN_TR * KNN_DC)   // floats per LDS buffer

// MODE 0: radius2[i] = the (k + 1)-th smallest squared distance within the row's own segment (L >= k + 1 list entries per lane)
// MODE 1: count[i] = #{ j : dist(i, j) <= rad[j] }, nearest2[i] = min_j dist(i, j)
template <int MODE, int L>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(int nq, int nr, int d, int k, int vec_q, int vec_r, const float* __restrict__ q,
                                                          const int32_t* __restrict__ q_off, const float* __restrict__ r,
                                                          const int32_t* __restrict__ r_off, const float* __restrict__ rad,
                                                          float* __restrict__ radius2, int32_t* __restrict__ count,
                                                          float* __restrict__ nearest2) {
  __shared__ __attribute__((aligned(16))) float smem[2 * KNN_TILE];          // two staged tiles; afterwards the merge area
  __shared__ float srad[2][KNN_TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, seg = blockIdx.y;
  int qs, qe, rs, re;
  knn_segment(q_off, seg, nq, &qs, &qe);
  knn_segment(r_off, seg, nr, &rs, &re);
  const long q0 = (long)qs + (long)blockIdx.x * KNN_QT;
  if (q0 >= qe) return;                                   // (the whole workgroup: no barrier has been met)
  const long qrow = q0 + lane;
  const bool q_ok = qrow < qe;
  const int nchunks = (d + KNN_DC - 1) / KNN_DC;
  const int m = re - rs;
  const int ntiles = (m + KNN_TR - 1) / KNN_TR;
  const int nsteps = ntiles * nchunks;                    // step = (tile, chunk), chunk fastest

  float qreg[KNN_DC];
  auto load_q = [&](int c) {
#pragma unroll
    for (int i = 0; i < KNN_DC; i += 4) {
      const float4 v = knn_load4(q, (size_t)qrow, d, c * KNN_DC + i, q_ok, vec_q != 0);
      qreg[i] = v.x; qreg[i + 1] = v.y; qreg[i + 2] = v.z; qreg[i + 3] = v.w;
    }
  };
  // staging: 1024 float4 per tile, two per thread
  float4 pf[2];
  float pf_rad = -1.f;
  auto fetch = [&](int step) {
    const int t = step / nchunks, c = step - t * nchunks;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int f = tid + KNN_THREADS * u, row = f >> 4, c4 = (f & 15) * 4;
      const long j = (long)rs + (long)t * KNN_TR + row;
      pf[u] = knn_load4(r, (size_t)j, d, c * KNN_DC + c4, j < re, vec_r != 0);
    }
    if (MODE == 1 && tid < KNN_TR) {
      const long j = (long)rs + (long)t * KNN_TR + tid;
      pf_rad = (rad != nullptr && j < re) ? rad[j] : -1.f;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int f = tid + KNN_THREADS * u;
      *(float4*)&smem[buf * KNN_TILE + f * 4] = pf[u];
    }
    if (MODE == 1 && tid < KNN_TR) srad[buf][tid] = pf_rad;
  };

  float list[L];
#pragma unroll
  for (int t = 0; t < L; ++t) list[t] = INFINITY;
  int cnt = 0;
  float mn = INFINITY;
  float acc[KNN_RW];

  if (nchunks == 1) load_q(0);
  if (nsteps > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    const int t = step / nchunks, c = step - t * nchunks;
    if (step + 1 < nsteps) fetch(step + 1);
    const int nvalid = min(KNN_TR, m - t * KNN_TR);        // rows of this tile that exist
    if (wave * KNN_RW < nvalid) {                          // (uniform per wavefront)
      if (nchunks > 1) load_q(c);
      if (c == 0) {
#pragma unroll
        for (int rr = 0; rr < KNN_RW; ++rr) acc[rr] = 0.f;
      }
      const float* tile = &smem[buf * KNN_TILE + wave * KNN_RW * KNN_DC];
#pragma unroll
      for (int i = 0; i < KNN_DC; i += 4) {
#pragma unroll
        for (int rr = 0; rr < KNN_RW; ++rr) {
          const float4 v = *(const float4*)&tile[rr * KNN_DC + i];
          float e;
          e = qreg[i] - v.x;     acc[rr] = fmaf(e, e, acc[rr]);
          e = qreg[i + 1] - v.y; acc[rr] = fmaf(e, e, acc[rr]);
          e = qreg[i + 2] - v.z; acc[rr] = fmaf(e, e, acc[rr]);
          e = qreg[i + 3] - v.w; acc[rr] = fmaf(e, e, acc[rr]);
        }
      }
      if (c == nchunks - 1) {
#pragma unroll
        for (int rr = 0; rr < KNN_RW; ++rr) {
          if (wave * KNN_RW + rr < nvalid) {               // (uniform: a row past the segment's end is zeros, not a reference)
            const float dist = acc[rr];
            if (MODE == 0) {
              if (__any(dist < list[L - 1])) {             // sorted insertion, unrolled: the list stays in registers
                float v = dist;
#pragma unroll
                for (int s = 0; s < L; ++s) {
                  const float lo = fminf(list[s], v), hi = fmaxf(list[s], v);
                  list[s] = lo;
                  v = hi;
                }
              }
            } else {
              cnt += dist <= srad[buf][wave * KNN_RW + rr] ? 1 : 0;      // (a negative radius never matches: dist >= 0)
              mn = fminf(mn, dist);
            }
          }
        }
      }
    }
    if (step + 1 < nsteps) stash(buf ^ 1);
    __syncthreads();
  }

  // merge the 8 wavefronts' results for the same 64 queries (the last barrier above freed the tiles)
  float* mf = smem;
  if (MODE == 0) {
    if (wave > 0) {
#pragma unroll
      for (int s = 0; s < L; ++s) mf[((wave - 1) * L + s) * 64 + lane] = list[s];
    }
    __syncthreads();
    if (wave == 0) {
      for (int w = 0; w < KNN_WAVES - 1; ++w) {
#pragma unroll
        for (int s2 = 0; s2 < L; ++s2) {
          float v = mf[(w * L + s2) * 64 + lane];
#pragma unroll
          for (int s = 0; s < L; ++s) {
            const float lo = fminf(list[s], v), hi = fmaxf(list[s], v);
            list[s] = lo;
            v = hi;
          }
        }
      }
      float out = -1.f;
      if (m > k) {
#pragma unroll
        for (int s = 0; s < L; ++s) out = s == k ? list[s] : out;
      }
      if (q_ok) radius2[qrow] = out;
    }
  } else {
    int* mi = (int*)(smem + KNN_WAVES * 64);
    if (wave > 0) {
      mf[(wave - 1) * 64 + lane] = mn;
      mi[(wave - 1) * 64 + lane] = cnt;
    }
    __syncthreads();
    if (wave == 0) {
      for (int w = 0; w < KNN_WAVES - 1; ++w) {
        mn = fminf(mn, mf[w * 64 + lane]);
        cnt += mi[w * 64 + lane];
      }
      if (q_ok) {
        if (count) count[qrow] = cnt;
        if (nearest2) nearest2[qrow] = mn;
      }
    }
  }
}

extern "C" {

int rcgan_knn_radius(rcgan_ctx* ctx, int n, int d, int k, int n_seg, const float* x, const int32_t* off, float* radius2) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool ok = n >= 1 && d >= 1 && d <= KNN_MAX_D && k >= 1 && k <= KNN_MAX_K && n_seg >= 1 && n_seg <= KNN_MAX_SEG && x && off && radius2 &&
                  ((uintptr_t)x & 3) == 0 && ((uintptr_t)off & 3) == 0 && ((uintptr_t)radius2 & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "n %d (>= 1), d %d (1..%d), k %d (1..%d), n_seg %d (1..%d), x / off / radius2 %s", n, d, KNN_MAX_D, k, KNN_MAX_K, n_seg,
             KNN_MAX_SEG, x && off && radius2 ? "given" : "NULL");
  const dim3 grid(cdiv(n, KNN_QT), n_seg), block(KNN_THREADS);
  const int vec = knn_vec(x, d);
#define KNN_RADIUS(L)                                                                                                              \
  hipLaunchKernelGGL((knn_kernel<0, L>), grid, block, 0, ctx->stream, n, n, d, k, vec, vec, x, off, x, off, (const float*)nullptr, radius2, \
                     (int32_t*)nullptr, (float*)nullptr)
  if (k <= 1) KNN_RADIUS(2);
  else if (k <= 5) KNN_RADIUS(6);
  else KNN_RADIUS(KNN_MAX_K + 1);
#undef KNN_RADIUS
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_ball_query(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const float* q, const int32_t* q_off, const float* r,
                     const int32_t* r_off, const float* r_radius2, int32_t* count, float* nearest2) {
  const bool ok = nq >= 1 && nr >= 1 && d >= 1 && d <= KNN_MAX_D && n_seg >= 1 && n_seg <= KNN_MAX_SEG && q && q_off && r && r_off &&
                  (r_radius2 || !count) && ((uintptr_t)q & 3) == 0 && ((uintptr_t)r & 3) == 0 && ((uintptr_t)q_off & 3) == 0 &&
                  ((uintptr_t)r_off & 3) == 0 && ((uintptr_t)r_radius2 & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)nearest2 & 3) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "nq %d, nr %d (>= 1), d %d (1..%d), n_seg %d (1..%d), q / q_off / r / r_off %s, r_radius2 %s (NULL only without count)", nq, nr,
             d, KNN_MAX_D, n_seg, KNN_MAX_SEG, q && q_off && r && r_off ? "given" : "NULL", r_radius2 ? "given" : "NULL");
  const dim3 grid(cdiv(nq, KNN_QT), n_seg), block(KNN_THREADS);
  hipLaunchKernelGGL((knn_kernel<1, 1>), grid, block, 0, ctx->stream, nq, nr, d, 0, knn_vec(q, d), knn_vec(r, d), q, q_off, r, r_off, r_radius2,
                     (float*)nullptr, count, nearest2);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
