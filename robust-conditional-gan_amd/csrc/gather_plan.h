// What the gather-GEMM family (conv_direct.hip: fp32 convolutions, 5x5 / stride-2 and transposed convolutions, dense layers, column sums)
// launches for a call, and with what geometry: the one place that decides it (conv_direct.hip and api.hip launch what this says).
// Free of HIP and of the environment: pure functions of the call's shape and of the switch values (GatherSwitches; conv_direct.hip
// reads the RCGAN_GG_* / RCGAN_NARROW_TWO_STEP / RCGAN_S2_LPT variables once and passes them in), so a stand-alone program can sweep it
// (tests/tools/gather_plan_sweep.cpp).
//
// decision                         function                      taken when
// -------------------------------  ----------------------------  ---------------------------------------------------------------------
// K-slices per workgroup (1/2/4)   gather_ks                     < ks_min_steps K-steps: 1; >= ks2_min_wgs workgroups: 2; else 4
// grid refusal                     gather_grid_ok                ceil(M / 64) and the z extent each <= 65535
// split reduction (fwd / dense dx) split_r_chunks, split_r_plan  fp32, < 128 tiles, >= 32 K-steps: up to 8 chunks of whole K-steps
// filter-gradient slabs            wgrad_splits, wgrad_plan      ceil(1024 / tiles) capped by ceil(M / 256) and 256, trimmed to whole
//                                  linear_wgrad_splits           dispatch rounds; dense: one chunk (no slabs) up to m = 1024
// column sums                      colsum_plan                   single kernel / 8-wide partials / narrow partials / 64-column partials
// small dense kernels              linear_tiny, linear_skinny    <= 65536 outputs over <= 4096 terms; n <= 16, k >= 512, m <= 65535
// operand vector width             gather_vec_of                 channel count and base address both multiples of 4 / 2 elements
// stride-2 data gradient           s2_classes, s2_route          parity classes; two-step / 16-lanes-per-pixel kernel / GEMM
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define GP_HD __host__ __device__ __forceinline__
#else
#define GP_HD inline
#endif

static inline long gp_cdiv(long a, long b) { return (a + b - 1) / b; }

// Division by a launch-invariant 32-bit divisor as multiply-high + shifts (Granlund-Montgomery, branch-free form):
// the operand decode of every K-step divides by the channel count and the filter width, ~30 VALU ops each when the
// compiler has to expand a general division.
struct FastDiv {
  unsigned d, m, s;
  GP_HD unsigned div(unsigned n) const {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned t = __umulhi(n, m);
#else
    const unsigned t = (unsigned)(((unsigned long long)n * m) >> 32);
#endif
    const unsigned q = (t + ((n - t) >> 1)) >> s;
    return d == 1 ? n : q;
  }
};
static inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f; f.d = d; f.m = 0; f.s = 0;
  if (d <= 1) return f;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;                       // ceil(log2 d)
  f.m = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.s = l - 1;
  return f;
}

// The switches, with their defaults.  conv_direct.hip fills one from the environment at its first launch.
struct GatherSwitches {
  int ks_min_steps = 8;      // RCGAN_GG_KS_MINSTEPS: K-steps from which a workgroup runs more than one K-slice
  int ks_force = 0;          // RCGAN_GG_KS: 1 / 2 force that many slices
  long ks2_min_wgs = 256;    // RCGAN_GG_KS2_MINWGS: workgroups from which two slices replace four
  int split_r = 1;           // RCGAN_GG_SPLIT_R: 0 off, 1 on (debug: 2 = convolutions only, 3 = dense layers only)
  int wgrad_fit = 1;         // RCGAN_GG_WGRAD_FIT: trim the filter-gradient split count to whole dispatch rounds
  int narrow_two_step = 1;   // RCGAN_NARROW_TWO_STEP: narrow stride-2 data gradients as dense products + col2im
  int s2_lpt = 1;            // RCGAN_S2_LPT: stride-2 parity classes longest first
};

#define GG_XBUF 2304         /* floats per operand buffer of the GEMM: max(64 x 36 K-major, 32 x 68 N-major) */
#define GG_RED_FLOATS 4096   /* floats one K-group leaves for the final sum: 4 waves x 16 registers x 64 lanes */
static_assert((4 - 1) * GG_RED_FLOATS <= 4 * 4 * GG_XBUF && (2 - 1) * GG_RED_FLOATS <= 2 * 4 * GG_XBUF,
              "the K-group reduction area lies inside the operand buffers");

// ---- launch_gemm --------------------------------------------------------------------------------------------------------------
// A grid the hardware takes: y = ceil(M / 64) row tiles, z = reduction chunks or parity classes (x = column tiles is far below its limit)
static inline bool gather_grid_ok(long M, long nz) { return gp_cdiv(M, 64) <= 65535 && nz <= 65535; }

// K-slices per workgroup.  Four K-slices per workgroup = 1024 threads = ONE workgroup per CU: a grid of more workgroups than CUs runs
// in whole rounds (392 workgroups: two, the second half empty).  Two slices = two workgroups per CU, the same K-steps per wavefront
// pair -- measured on the MNIST iteration (B = 256), per launch: 1568 workgroups 214 -> 177 us, 1666 111 -> 84, 392 170 -> 161; but
// 196 workgroups 46 -> 53, 128 44 -> 51 (fewer workgroups than CUs: the four slices are the parallelism).
static inline int gather_ks(long r_chunk, long wgs, const GatherSwitches& sw) {
  const long steps = (r_chunk + 31) / 32;
  if (sw.ks_force == 2) return 2;
  if (sw.ks_force == 1) return 1;
  if (steps >= sw.ks_min_steps) return wgs >= sw.ks2_min_wgs ? 2 : 4;
  return 1;
}
static inline long gather_wgs(long M, long N, long nz) { return gp_cdiv(N, 64) * gp_cdiv(M, 64) * nz; }

// ---- reduction chunks -----------------------------------------------------------------------------------------------------------
struct GatherChunks { long r_chunk; int nz; };      // chunk z covers [z * r_chunk, min(R, (z + 1) * r_chunk)), nz of them

// Forward / data-gradient GEMMs with few output tiles and a long reduction: the number of chunks the reduction is cut into (1: no split).
// kind 1: convolution forward, 2: dense data gradient
static inline int split_r_chunks(long M, long N, long R, int kind, const GatherSwitches& sw) {
  const long tiles = gp_cdiv(M, 64) * gp_cdiv(N, 64), steps = (R + 31) / 32;
  const int en = sw.split_r;
  if (!en || (en == 2 && kind != 1) || (en == 3 && kind != 2) || tiles >= 128 || steps < 32) return 1;
  long nz = 256 / tiles;
  if (nz > steps / 8) nz = steps / 8;       // >= 8 K-steps per chunk
  if (nz > 8) nz = 8;
  return nz < 2 ? 1 : (int)nz;
}
// chunks of whole K-steps (32) for a planned count; the final count may be lower
static inline GatherChunks split_r_plan(long R, int nz) {
  GatherChunks c;
  c.r_chunk = (((R + nz - 1) / nz) + 31) / 32 * 32;
  c.nz = (int)gp_cdiv(R, c.r_chunk);
  return c;
}

// the number of r-splits of a filter-gradient GEMM ([K x Cout] outputs over M rows) so the grid fills the chip
static inline int wgrad_splits(long K, long Cout, long M, const GatherSwitches& sw) {
  long tiles = gp_cdiv(K, 64) * gp_cdiv(Cout, 64);
  long want = (1024 + tiles - 1) / tiles;
  long maxs = (M + 255) / 256;
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  if (want > 256) want = 256;
  // (round 6) whole rounds: such a grid runs two 512-thread workgroups per CU (gather_ks: two K-slices, 74 KB of LDS each), 512 at
  // a time on 256 CUs.  tiles x splits just above a multiple of 512 -- the MNIST generator's 5x5 transposed convolution: 150 tiles
  // x 7 splits = 1050 -- pays a whole extra round for a few workgroups; one split less (900: two rounds of 17 % longer workgroups)
  // is the shorter launch.  RCGAN_GG_WGRAD_FIT=0: the plain ceil(1024 / tiles).
  if (sw.wgrad_fit && want > 1 && tiles * want >= 512) {
    const long over = (tiles * want) % 512;
    if (over != 0 && over * 4 < 512) {               // the last round less than a quarter full
      long w2 = want;
      while (w2 > 1 && (tiles * w2) % 512 != 0 && ((tiles * w2) % 512) * 4 < 512 && tiles * w2 > 512) --w2;
      // accept when the rounds saved outweigh the longer workgroups: rounds(w2) / w2 < rounds(want) / want
      const long r1 = (tiles * want + 511) / 512, r2 = (tiles * w2 + 511) / 512;
      if (r2 * want < r1 * w2) want = w2;
    }
  }
  return (int)want;
}
// dense filter gradient: up to 1024 batch rows one chunk, straight into the gradient (no slabs)
static inline int linear_wgrad_splits(long m, long k, long n, const GatherSwitches& sw) { return m <= 1024 ? 1 : wgrad_splits(k, n, m, sw); }
// chunks of whole 16-row groups for a planned count; the final count may be lower
static inline GatherChunks wgrad_plan(long M, int nz) {
  GatherChunks c;
  c.r_chunk = ((M + nz - 1) / nz + 15) / 16 * 16;
  c.nz = (int)gp_cdiv(M, c.r_chunk);
  return c;
}

// ---- column sums ------------------------------------------------------------------------------------------------------------------
enum ColsumRoute {
  COLSUM_SINGLE,      // colsum_kernel over all rows
  COLSUM_VEC,         // colsum_vec_partial_kernel (8 columns per thread; c % 8 == 0 and (c / 8) | 256) + colsum_kernel over the partials
  COLSUM_NARROW,      // colsum_narrow_partial_kernel (c <= 8) + colsum_kernel
  COLSUM_PARTIAL      // colsum_partial_kernel (64 columns per workgroup, 2048 rows per block) + colsum_kernel
};
struct ColsumPlan { ColsumRoute route; long rows_per_blk; long nb; };      // nb partial rows of c floats (0: none)

// floats every caller reserves for the partial rows of a [rows][c] column sum: at most 1024 rows on the doubling routes, ceil(rows /
// 2048) on the plain one
static inline size_t colsum_partial_floats(long rows, long c) { return (size_t)(gp_cdiv(rows, 2048) + 1024) * (size_t)c; }
// ... as the 256-byte-rounded tail that rcgan_deconv2d_bwd_weight[_concat] put at the end of their workspace
static inline size_t colsum_tail_bytes(long rows, long c) { return (colsum_partial_floats(rows, c) * sizeof(float) + 255) / 256 * 256; }

static inline ColsumPlan colsum_plan(long rows, int c, bool have_ws) {
  ColsumPlan p = {COLSUM_SINGLE, rows, 0};
  if (have_ws && rows >= 2048 && c % 8 == 0 && c <= 256 && 256 % (c / 8) == 0) {
    p.route = COLSUM_VEC; p.rows_per_blk = 256;
    while ((rows + p.rows_per_blk - 1) / p.rows_per_blk > 1024) p.rows_per_blk *= 2;
    p.nb = gp_cdiv(rows, p.rows_per_blk);
    return p;
  }
  if (have_ws && rows >= 4096 && c <= 8) {
    p.route = COLSUM_NARROW; p.rows_per_blk = 1024;
    while ((rows + p.rows_per_blk - 1) / p.rows_per_blk > 1024) p.rows_per_blk *= 2;
    p.nb = gp_cdiv(rows, p.rows_per_blk);
    return p;
  }
  if (rows <= 4096 || !have_ws) return p;
  p.route = COLSUM_PARTIAL; p.rows_per_blk = 2048; p.nb = gp_cdiv(rows, 2048);
  return p;
}

// ---- workspaces ---------------------------------------------------------------------------------------------------------------------
// filter gradient of a convolution: [K x Cout] outputs over M rows: the slabs, then the column-sum partials of the bias gradient
static inline size_t gather_wgrad_slab_bytes(long K, long Cout, long M, const GatherSwitches& sw) {
  return (size_t)wgrad_splits(K, Cout, M, sw) * K * Cout * sizeof(float);
}
static inline size_t gather_wgrad_ws_bytes(long K, long Cout, long M, const GatherSwitches& sw) {
  return gather_wgrad_slab_bytes(K, Cout, M, sw) + colsum_partial_floats(M, Cout) * sizeof(float) + 256;
}
// dense filter gradient: slabs only when the reduction is split
static inline size_t linear_wgrad_slab_bytes(long m, long k, long n, const GatherSwitches& sw) {
  const int nz = linear_wgrad_splits(m, k, n, sw);
  return (size_t)(nz > 1 ? nz : 0) * k * n * sizeof(float);
}
static inline size_t linear_wgrad_plan_bytes(long m, long k, long n, const GatherSwitches& sw) {
  return linear_wgrad_slab_bytes(m, k, n, sw) + colsum_partial_floats(m, n) * sizeof(float) + 256;
}
// label-column filter gradient (direct_wgrad_cols): slabs [nz][K][c1] | D [RG][N][K] | chunk partials [ceil(N / 8)][K][c2]
#define WGRAD_LABEL_RG 4        /* row groups: a sample's image rows ih = rg, rg + 4, ... go to workgroup (n, rg) */
#define WGRAD_LABEL_PER_CHUNK 8 /* samples per chunk of the label-column product */
struct WgradColsLayout { size_t slab, D, partial, end; };      // offsets in floats
static inline WgradColsLayout gather_wgrad_cols_layout(long K, long c1, long c2, long M, long N, const GatherSwitches& sw) {
  WgradColsLayout l;
  l.slab = 0;
  l.D = (size_t)wgrad_splits(K, c1, M, sw) * K * c1;
  l.partial = l.D + (size_t)WGRAD_LABEL_RG * N * K;
  l.end = l.partial + (size_t)gp_cdiv(N, WGRAD_LABEL_PER_CHUNK) * K * c2;
  return l;
}
static inline size_t gather_wgrad_cols_ws_bytes(long K, long c1, long c2, long M, long N, const GatherSwitches& sw) {
  return gather_wgrad_cols_layout(K, c1, c2, M, N, sw).end * sizeof(float) + 1024;
}

// ---- small dense kernels -------------------------------------------------------------------------------------------------------------
// linear_tiny_kernel: one thread per output element
static inline bool linear_tiny(long outputs, long red) { return outputs <= 65536 && red <= 4096; }
// linear_skinny_fwd_kernel: one workgroup per row splits K over its 256 threads
static inline bool linear_skinny(long m, long k, long n) { return n <= 16 && k >= 512 && m <= 65535; }

// ---- operand vector width ---------------------------------------------------------------------------------------------------------
// elements per load along the contiguous dimension (c of them per run) from base address a
static inline int gather_vec_of(uintptr_t a, long c, size_t elem) {
  if (c % 4 == 0 && a % (4 * elem) == 0) return 4;
  if (c % 2 == 0 && a % (2 * elem) == 0) return 2;
  return 1;
}

// ---- stride-2 data gradient -------------------------------------------------------------------------------------------------------
// One input-pixel PARITY CLASS (ih % 2, iw % 2): only the taps kh = kh0 + 2*jh, kw = kw0 + 2*jw reach an output pixel.
struct S2Cls { int ph, pw, Hp, Wp, kh0, kw0, nkh, nkw, dh, dwc; long M, R; FastDiv dnkw; };
struct S2Table { S2Cls cls[4]; };
struct S2Plan { S2Table tab; int ncls; long maxM, maxR; };

// the (up to) four classes of an [N, H, W] input under a KH x KW stride-2 filter with padding (PT, PL) and Cout reduction channels;
// unused table slots repeat class 0
static inline S2Plan s2_classes(int N, int H, int W, int Cout, int KH, int KW, int PT, int PL, const GatherSwitches& sw) {
  S2Plan p;
  p.ncls = 0; p.maxM = 0; p.maxR = 0;
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      S2Cls c;
      c.ph = ph; c.pw = pw; c.Hp = (H - ph + 1) / 2; c.Wp = (W - pw + 1) / 2;
      if (c.Hp <= 0 || c.Wp <= 0) continue;
      c.kh0 = (ph + PT) % 2; c.kw0 = (pw + PL) % 2;
      c.nkh = KH > c.kh0 ? (KH - c.kh0 + 1) / 2 : 0;
      c.nkw = KW > c.kw0 ? (KW - c.kw0 + 1) / 2 : 0;
      c.dh = (ph + PT - c.kh0) / 2; c.dwc = (pw + PL - c.kw0) / 2;
      if (c.nkw == 0) { c.nkw = 1; c.nkh = 0; }          // keeps the divisions defined; R = 0: outputs are bias / 0
      c.dnkw = make_fastdiv(c.nkw);
      c.M = (long)N * c.Hp * c.Wp; c.R = (long)c.nkh * c.nkw * Cout;
      if (c.M > p.maxM) p.maxM = c.M;
      if (c.R > p.maxR) p.maxR = c.R;
      p.tab.cls[p.ncls++] = c;
    }
  if (p.ncls == 0) { p.tab = S2Table(); return p; }
  // (round 6) longest class first: grid.z is the slowest dispatch index, and with a 5x5 filter the classes reduce over 4, 6, 6 and 9
  // taps -- in (ph, pw) order the 9-tap workgroups started last and the launch ended on them alone.  RCGAN_S2_LPT=0: (ph, pw) order.
  if (sw.s2_lpt) std::stable_sort(p.tab.cls, p.tab.cls + p.ncls, [](const S2Cls& a, const S2Cls& b) { return a.R * a.M > b.R * b.M; });
  for (int q = p.ncls; q < 4; ++q) p.tab.cls[q] = p.tab.cls[0];
  return p;
}

enum S2Route {
  S2_TWO_STEP,      // fp32, one or two output channels, no ReLU mask: products per source pixel (linear_dgrad) + col2im_s2_kernel
  S2_NARROW,        // dgrad_s2_narrow_kernel: <= 4 output channels, the filter slice in <= 48 KiB of LDS
  S2_GEMM           // the gather GEMM, class = grid.z
};
#define S2_TWO_STEP_MAX_BYTES ((size_t)1 << 30)
#define S2_NARROW_MAX_LDS (48 * 1024)
// ncols = output channels of the data gradient (the descriptor's cin), cout = its reduction channels; two_step_bytes = the products'
// scratch, [n * oh * ow][kh * kw * cin] floats
static inline S2Route s2_route(bool f32, long ncols, bool has_mask, long cout, size_t two_step_bytes, long maxR, const GatherSwitches& sw) {
  if (f32 && sw.narrow_two_step && ncols <= 2 && !has_mask && cout >= 32 && two_step_bytes <= S2_TWO_STEP_MAX_BYTES) return S2_TWO_STEP;
  if (ncols <= 4 && maxR > 0 && (size_t)maxR * ncols * sizeof(float) <= S2_NARROW_MAX_LDS) return S2_NARROW;
  return S2_GEMM;
}
