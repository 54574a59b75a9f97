// Nearest reference image of every query image in pixel space (neighbours.py: copy rate, nearest-neighbour distance test, leave-one-out
// 1-NN accuracy), EXACT: best[i] = min_j ((uint64)dist2(i, j) << 32 | j) over the reference rows j of query row i's segment, with
// dist2 the integer sum of squared pixel differences.  Rows are raw uint8 pixels, grouped into contiguous segments as in knn.hip /
// ksum.hip: segment s of the queries only ever meets segment s of the references.
//
// Arithmetic.  A staged dword is centred with one xor: x ^ 0x80 read as int8 is x - 128, so a = q - 128 and b = r - 128 lie in
// [-128, 127] and a - b = q - r.  dist2 = |a|^2 + |b|^2 - 2 a.b, all int32: the inner products on the integer matrix cores
// (v_mfma_i32_32x32x32_i8, int32 accumulate), the squared norms from the same staged dwords with the 4 x int8 dot instruction
// (v_dot4_i32_i8) on the vector units.  The int32 bound, for d <= 12288 = 3 * 2^12 features:
//   every product of two centred values is at most 128 * 128 = 2^14 in magnitude, so every partial sum of a norm or of an inner
//   product, in any order, is at most d * 2^14 <= 201 326 592 < 2^28 in magnitude: the MFMA accumulator and the dot4 chains never wrap;
//   |a|^2 + |b|^2 <= 2 d 2^14 = 402 653 184 and |2 a.b| <= 402 653 184, so the one sum and the one difference that form dist2 stay
//   below 805 306 368 < 2^30 in magnitude: no intermediate comes within a factor of 2 of 2^31;
//   the result is the exact value, 0 <= dist2 <= d * 255^2 <= 799 027 200 < 2^30, so it also fits the upper 32 bits of the key and is
//   never 0xFFFFFFFF, the value that stands for "no candidate".
// Features past d (d is a multiple of 16; a chunk is 128) are staged as centred zero, which adds exactly nothing to a norm or an
// inner product.  Rows past a segment's end are staged as centred zero too and masked in the epilogue by their index (a centred-zero
// row is the legal image of all-128 pixels, so the data cannot mark them).
//
// grid = (tiles of 128 query rows, segments, reference splits), 256 threads.  A workgroup holds its 128 query rows against successive
// tiles of 128 reference rows of its split's range; both tiles are staged through LDS in chunks of 128 features, double-buffered (the
// next chunk's global loads are in flight while this one is multiplied -- nothing reads them before the stash -- one barrier per
// chunk).  The references are the M side of the MFMA and the queries the N side, so a lane's 16 accumulator entries are 16 reference rows of ONE query (column lane % 32):
// wavefront w takes reference rows 64 (w / 2) .. + 63 against queries 64 (w % 2) .. + 63 as 2 x 2 blocks of 32 x 32.  A dot product
// does not care in which order the features are paired: of a k-step of 32 features the lower half-wave takes bytes 0..15 and the
// upper bytes 16..31 on BOTH operands (one 16-byte LDS read each; row stride 144 bytes: conflict-free), so only the C/D map and
// "lane -> row (A) / column (B)" are relied on, never the i8 k order inside a fragment.
// The staging threads also own the norms: thread t always stages piece t % 8 of rows t / 8 + 32 u, so it adds the dot4 of its dwords
// with themselves to four running sums per operand; after a tile's last chunk eight lanes are added with lane exchanges and the
// row's norm goes to LDS (the reference norms double-buffered by tile parity, the query norms taken on the first tile only).
// Epilogue per reference tile: a lane meets its candidates in ascending row order, so a strict < on the distance keeps the lowest
// index; rows past the segment's end and the excluded row compare as 0xFFFFFFFF.  The running minimum (distance, index) per query
// column stays in registers across the whole reference range.  At the end the two half-waves are merged with a lane exchange, the two
// wavefronts that share a query through LDS, and each query row costs ONE 64-bit atomic minimum (a vector integer atomic: the result
// does not depend on the order or on the split) into best, which a fill launch on the same stream has set to all-ones for every row
// inside a segment.  Rows outside every segment are touched by neither launch.
//
// The split count is chosen on the host from nq, nr and n_seg alone (the offsets live on the device): about 1024 workgroups, two
// rounds of the 512 that are resident, but at least 4 reference tiles per split so that the staging prologue is amortised.
//
// nn_u8_kernel: 231 VGPRs (of the 256 that two wavefronts per SIMD leave each), no scratch, 77 312 bytes of LDS: two workgroups (8
// wavefronts) per CU, so that one's epilogue and barriers run under the other's MFMAs.  nn_u8_fill_kernel: 4 VGPRs, no LDS.
#include "seg_rows.h"

#define NN_T 128                       // rows per staged tile, queries and references alike
#define NN_THREADS 256
#define NN_KC 128                      // features (bytes) per staged chunk: four k-steps of 32
#define NN_LD (NN_KC + 16)             // LDS row stride (bytes): 16 lanes of a 16-byte read land on 16 different bank quads
#define NN_TILE (NN_T * NN_LD)         // bytes per staged operand tile
#define NN_BUF (2 * NN_TILE)           // one buffer: the reference tile, then the query tile
#define NN_MIN_D 16
#define NN_MAX_D 12288
#define NN_MAX_SPLIT 64
#define NN_MIN_TILES_PER_SPLIT 4
#define NN_TARGET_GROUPS 1024
#define NN_CENTRE 0x80808080u

typedef __attribute__((ext_vector_type(4))) int nn_i32x4_t;
typedef __attribute__((ext_vector_type(16))) int nn_i32x16_t;

// |v|^2 of the 16 centred int8 values of v, added to s
__device__ __forceinline__ int nn_norm16(uint4 v, int s) {
  s = __builtin_amdgcn_sdot4((int)v.x, (int)v.x, s, false);
  s = __builtin_amdgcn_sdot4((int)v.y, (int)v.y, s, false);
  s = __builtin_amdgcn_sdot4((int)v.z, (int)v.z, s, false);
  return __builtin_amdgcn_sdot4((int)v.w, (int)v.w, s, false);
}

// 16 raw pixels -> 16 centred int8 values (x ^ 0x80 read as int8 is x - 128); centred zero when the piece does not exist
__device__ __forceinline__ uint4 nn_centre(uint4 v, bool exists) {
  return make_uint4(exists ? v.x ^ NN_CENTRE : 0u, exists ? v.y ^ NN_CENTRE : 0u, exists ? v.z ^ NN_CENTRE : 0u, exists ? v.w ^ NN_CENTRE : 0u);
}

// every row inside a query segment starts as "no candidate"
__global__ __launch_bounds__(256) void nn_u8_fill_kernel(int nq, const int32_t* __restrict__ q_off, unsigned long long* __restrict__ best) {
  int qs, qe;
  knn_segment(q_off, blockIdx.y, nq, &qs, &qe);
  const long i = (long)qs + (long)blockIdx.x * 256 + threadIdx.x;
  if (i < qe) best[i] = ~0ull;
}

__global__ __launch_bounds__(NN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void nn_u8_kernel(
    int nq, int nr, int d, const uint8_t* __restrict__ q, const int32_t* __restrict__ q_off, const uint8_t* __restrict__ r,
    const int32_t* __restrict__ r_off, int exclude, unsigned long long* __restrict__ best) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * NN_BUF + 3 * NN_T * 4 + 4 * 64 * 8];
  int* rnorm = (int*)(smem + 2 * NN_BUF);                                   // [2][NN_T]: by the parity of the tile
  int* qnorm = rnorm + 2 * NN_T;                                            // [NN_T]
  unsigned long long* merge = (unsigned long long*)(qnorm + NN_T);          // [4 wavefronts][64 queries]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, seg = blockIdx.y;
  const int col = lane & 31, half = lane >> 5, wq = wave & 1, wr = wave >> 1;
  int qs, qe, rs, re;
  knn_segment(q_off, seg, nq, &qs, &qe);
  knn_segment(r_off, seg, nr, &rs, &re);
  const long q0 = (long)qs + (long)blockIdx.x * NN_T;
  if (q0 >= qe) return;                                   // (the whole workgroup: no barrier has been met)
  const int ntiles = (re - rs + NN_T - 1) / NN_T;
  const int per_split = (ntiles + (int)gridDim.z - 1) / (int)gridDim.z;
  const int t0 = (int)blockIdx.z * per_split, t1 = min(ntiles, t0 + per_split);
  if (t0 >= t1) return;                                   // (an empty reference range: the fill launch has written "no candidate")
  const int nchunks = (d + NN_KC - 1) / NN_KC;
  const int nsteps = (t1 - t0) * nchunks;                 // step = (tile, chunk), chunk fastest

  // staging: 1024 16-byte pieces per operand tile, four per thread, always of the same four rows
  const int srow = tid >> 3, spiece = tid & 7;
  uint4 pr[4], pq[4];
  int rn[4] = {0, 0, 0, 0}, qn[4] = {0, 0, 0, 0};
  // (a piece that does not exist is loaded from a clamped address inside the tensor and replaced by centred zero when it is stashed:
  // no branch around a load, and nothing between the loads and the MFMAs that has to wait for them)
  auto fetch = [&](int step) __attribute__((always_inline)) {
    const int t = step / nchunks, c = step - t * nchunks;
    const int cbc = min(c * NN_KC + spiece * 16, d - 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long j = (long)rs + (long)(t0 + t) * NN_T + srow + 32 * u;
      const long i = q0 + srow + 32 * u;
      pr[u] = *(const uint4*)(r + (size_t)min(j, (long)re - 1) * (size_t)d + cbc);
      pq[u] = *(const uint4*)(q + (size_t)min(i, (long)qe - 1) * (size_t)d + cbc);
    }
  };
  auto stash = [&](int step) __attribute__((always_inline)) {
    const int t = step / nchunks, c = step - t * nchunks;
    const bool in_d = c * NN_KC + spiece * 16 < d;          // (d is a multiple of 16: a piece lies inside a row or past its end)
    unsigned char* base = smem + (step & 1) * NN_BUF + srow * NN_LD + spiece * 16;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long j = (long)rs + (long)(t0 + t) * NN_T + srow + 32 * u;
      const long i = q0 + srow + 32 * u;
      const uint4 b = nn_centre(pr[u], in_d & (j < re)), a = nn_centre(pq[u], in_d & (i < qe));
      rn[u] = nn_norm16(b, c == 0 ? 0 : rn[u]);
      if (t == 0) qn[u] = nn_norm16(a, qn[u]);
      *(uint4*)(base + 32 * u * NN_LD) = b;
      *(uint4*)(base + NN_TILE + 32 * u * NN_LD) = a;
    }
    if (c == nchunks - 1) {                               // the tile's norms are complete: eight lanes per row
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int s = rn[u], p = qn[u];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
        p += __shfl_xor(p, 1); p += __shfl_xor(p, 2); p += __shfl_xor(p, 4);
        if (spiece == 0) {
          rnorm[(t & 1) * NN_T + srow + 32 * u] = s;
          if (t == 0) qnorm[srow + 32 * u] = p;
        }
      }
    }
  };

  nn_i32x16_t acc[2][2];                                  // [reference block][query block]
  unsigned bestd[2] = {~0u, ~0u}, bestj[2] = {~0u, ~0u};  // per query block: the running minimum of this lane's candidates
  fetch(0);
  stash(0);                                               // (waits for every load so far: the loop starts with none in flight)
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int t = step / nchunks, c = step - t * nchunks;
    if (step + 1 < nsteps) fetch(step + 1);
    if (c == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[0][0][e] = acc[0][1][e] = acc[1][0][e] = acc[1][1][e] = 0;
    }
    const int nks = min(NN_KC / 32, (d - c * NN_KC + 31) / 32);               // k-steps of this chunk that hold features
    const unsigned char* ra = smem + (step & 1) * NN_BUF + (wr * 64 + col) * NN_LD + half * 16;
    const unsigned char* qb = smem + (step & 1) * NN_BUF + NN_TILE + (wq * 64 + col) * NN_LD + half * 16;
    auto kstep = [&](int ks) __attribute__((always_inline)) {
      const nn_i32x4_t a0 = *(const nn_i32x4_t*)(ra + ks * 32), a1 = *(const nn_i32x4_t*)(ra + 32 * NN_LD + ks * 32);
      const nn_i32x4_t b0 = *(const nn_i32x4_t*)(qb + ks * 32), b1 = *(const nn_i32x4_t*)(qb + 32 * NN_LD + ks * 32);
      acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
    };
    kstep(0);
    if (nks > 1) kstep(1);
    if (nks > 2) kstep(2);
    if (nks > 3) kstep(3);
    __builtin_amdgcn_sched_barrier(0);                      // (keeps the epilogue's and the stash's registers out of the MFMA phase)
    if (c == nchunks - 1) {
      const long tbase = (long)rs + (long)(t0 + t) * NN_T;                   // the global row of this tile's row 0
      const int nvalid = (int)min((long)NN_T, (long)re - tbase);             // rows of this tile that exist
      const int* rnp = rnorm + (t & 1) * NN_T;
#pragma unroll
      for (int bq = 0; bq < 2; ++bq) {
        const int ql = wq * 64 + bq * 32 + col;
        const int qn2 = qnorm[ql];
        // the tile row that is this lane's own query (exclude_same_row), if it is in this tile; else no row
        const long own = q0 + ql - tbase;
        const int skip = exclude && own >= 0 && own < NN_T ? (int)own : -1;
#pragma unroll
        for (int br = 0; br < 2; ++br) {
          __builtin_amdgcn_sched_barrier(0);               // (one 32 x 32 block at a time: the next tile's staged loads stay in registers)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int row0 = wr * 64 + br * 32 + 8 * g + 4 * half;           // the MFMA's C/D map: the reference row of entry 4 g
            const nn_i32x4_t n4 = *(const nn_i32x4_t*)&rnp[row0];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int row = row0 + i;
              const unsigned dist = (unsigned)(qn2 + n4[i] - 2 * acc[br][bq][4 * g + i]);
              const unsigned cand = ((row < nvalid) & (row != skip)) ? dist : ~0u;    // (& not &&: a select, no branch per entry)
              const bool nearer = cand < bestd[bq];        // (rows arrive in ascending order: strict < keeps the lowest index)
              bestd[bq] = nearer ? cand : bestd[bq];
              bestj[bq] = nearer ? (unsigned)tbase + (unsigned)row : bestj[bq];
            }
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (step + 1 < nsteps) stash(step + 1);
    __syncthreads();
  }

  // merge: the two half-waves by a lane exchange, the two wavefronts of a query through LDS, the splits by one atomic per row
#pragma unroll
  for (int bq = 0; bq < 2; ++bq) {
    unsigned long long key = ((unsigned long long)bestd[bq] << 32) | bestj[bq];
    const unsigned long long other = __shfl_xor(key, 32);
    key = other < key ? other : key;
    if (half == 0) merge[wave * 64 + bq * 32 + col] = key;
  }
  __syncthreads();
  if (tid < NN_T) {
    const int w = tid >> 6, c = tid & 63;
    const unsigned long long k0 = merge[w * 64 + c], k1 = merge[(2 + w) * 64 + c];
    const unsigned long long key = k1 < k0 ? k1 : k0;
    if (q0 + tid < qe && key != ~0ull) atomicMin(&best[q0 + tid], key);
  }
}

extern "C" {

int rcgan_nn_u8(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const uint8_t* q, const int32_t* q_off, const uint8_t* r,
                const int32_t* r_off, int exclude_same_row, uint64_t* best) {
  // (the argument checks come first and need no context: a bad call is refused even where no device exists)
  const bool ok = nq >= 1 && nr >= 1 && d >= NN_MIN_D && d <= NN_MAX_D && (d & 15) == 0 && n_seg >= 1 && n_seg <= KNN_MAX_SEG && q && q_off && r &&
                  r_off && best && ((uintptr_t)q & 15) == 0 && ((uintptr_t)r & 15) == 0 && ((uintptr_t)q_off & 3) == 0 &&
                  ((uintptr_t)r_off & 3) == 0 && ((uintptr_t)best & 7) == 0;
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, ok, "nq %d, nr %d (>= 1), d %d (%d..%d, a multiple of 16), n_seg %d (1..%d), q / q_off / r / r_off / best %s (q, r 16-byte, best 8-byte aligned)",
             nq, nr, d, NN_MIN_D, NN_MAX_D, n_seg, KNN_MAX_SEG, q && q_off && r && r_off && best ? "given" : "NULL");
  const int q_tiles = cdiv(nq, NN_T) + n_seg - 1, r_tiles = cdiv(nr, NN_T);      // (upper bounds: the offsets live on the device)
  const int split = std::max(1, std::min(std::min(cdiv(NN_TARGET_GROUPS, q_tiles), r_tiles / NN_MIN_TILES_PER_SPLIT), NN_MAX_SPLIT));
  hipLaunchKernelGGL(nn_u8_fill_kernel, dim3(cdiv(nq, 256), n_seg), dim3(256), 0, ctx->stream, nq, q_off, (unsigned long long*)best);
  RC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(nn_u8_kernel, dim3(cdiv(nq, NN_T), n_seg, split), dim3(NN_THREADS), 0, ctx->stream, nq, nr, d, q, q_off, r, r_off,
                     exclude_same_row != 0 ? 1 : 0, (unsigned long long*)best);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
