// Stand-alone sweep of the gather-GEMM family's launch decisions (csrc/gather_plan.h): host code only, nothing of HIP.
// tests/test_gather_plan_cpu.py builds it with the host compiler and -fsanitize=address,undefined and runs it as a child process.
//
//   gather_plan_sweep sweep   every decision over the grid below, for the default switches and for each switch off; prints one line per
//                             violated invariant (the first MAX_SHOWN of each kind), a summary, and exits 1 if anything was violated
//   gather_plan_sweep cases   reads the case lines of tests/test_gpu_gather_edges.py from standard input
//                                 conv   <dtype> n h w cin cout k s mask off      rcgan_conv2d_* (forced onto the gather GEMM) on that descriptor
//                                 deconv <dtype> n h w cin cout k s ncols tail    rcgan_deconv2d_* on the descriptor of the convolution it transposes
//                                 linear <dtype> m k n                            rcgan_linear_*
//                                 concat <dtype> n h w cin c1 c2 k s              rcgan_deconv2d_bwd_weight_concat (c1 real + c2 label columns)
//                             (dtype f32 | h16; mask: a ReLU mask on the data gradient; off: x and dy start that many elements past a 256-byte
//                             boundary; ncols: rcgan_deconv2d_bwd_data_cols, 0 = all; tail: the workspace holds the column-sum tail) and prints
//                             the branch each of the four calls takes, default switches:
//                                 case <kind> fwd=... dgrad=... wgrad=... dbias=... [vec=x<v>dy<v>] [tail=<bytes>] [chunks=<n>]
//                             (vec: the vector widths of the x and dy fetches; tail: colsum_tail_bytes; chunks: sample chunks of the label columns)
//
// The entry points of conv_direct.hip / api.hip are mirrored here (conv_fwd_branch, conv_dgrad_branch, wgrad_branch, ...): which shape they hand to the header.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../robust-conditional-gan_amd/csrc/gather_plan.h"

static const int MAX_SHOWN = 6;
static std::map<std::string, long> g_violations;
static long g_checked = 0;

static void violated(const char* what, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0) {
  long& n = g_violations[what];
  if (n++ < MAX_SHOWN) {
    printf("VIOLATION %s: ", what);
    printf(fmt, a, b, c, d);
    printf("\n");
  }
}
#define CHECK(cond, what, fmt, ...) do { ++g_checked; if (!(cond)) violated(what, fmt, __VA_ARGS__); } while (0)

// SAME padding of csrc/common.h
static void same_pad(int in, int k, int s, int* out, int* before) {
  int o = (in + s - 1) / s, tot = (o - 1) * s + k - in;
  if (tot < 0) tot = 0;
  *out = o; *before = tot / 2;
}

// chunks [z * r_chunk, min(R, (z + 1) * r_chunk)) for z < nz cover [0, R) once, none empty
static bool covers_once(long R, const GatherChunks& c) { return c.nz >= 1 && c.r_chunk >= 1 && (long)c.nz * c.r_chunk >= R && (long)(c.nz - 1) * c.r_chunk < R; }

// ---- sweep ----------------------------------------------------------------------------------------------------------------------
static const long SIZES[] = {1, 2, 3, 7, 8, 10, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 138, 200, 255, 256, 257, 511, 512, 513, 991, 992, 993, 1023, 1024,
                             1025, 1567, 1568, 2047, 2048, 2049, 2056, 3200, 3850, 4095, 4096, 4097, 6272, 8127, 8128, 8129, 16384, 65535, 65536, 65537, 262143,
                             262144, 262145, 1048575, 1048576, 1048577, 2097153, 4194240, 4194304};
static const int NSIZES = sizeof(SIZES) / sizeof(SIZES[0]);

static void sweep_fastdiv() {
  std::vector<unsigned> ds;
  for (unsigned d = 1; d <= 4096; ++d) ds.push_back(d);
  for (int k = 13; k <= 31; ++k) { ds.push_back((1u << k) - 1); ds.push_back(1u << k); ds.push_back((1u << k) + 1); }
  unsigned long long seed = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (unsigned)(seed >> 16); };
  for (unsigned d : ds) {
    const FastDiv f = make_fastdiv(d);
    const unsigned qmax = 0xffffffffu / d;
    unsigned ns[48];
    int c = 0;
    ns[c++] = 0; ns[c++] = d - 1; ns[c++] = d; ns[c++] = 0x80000000u; ns[c++] = 0xffffffffu;
    const unsigned qs[4] = {2u, qmax / 2 + 1, qmax ? qmax : 1u, qmax > 1 ? qmax - 1 : 1u};
    for (unsigned q : qs) { ns[c++] = q * d - 1; ns[c++] = q * d; }
    while (c < 48) ns[c++] = rnd();
    for (int i = 0; i < c; ++i) CHECK(f.div(ns[i]) == ns[i] / d, "fastdiv", "d %ld n %ld got %ld", (long)d, (long)ns[i], (long)f.div(ns[i]));
  }
}

static void sweep_gemm(const GatherSwitches& sw) {
  for (int a = 0; a < NSIZES; ++a)
    for (int b = 0; b < NSIZES; ++b) {
      const long M = SIZES[a], N = SIZES[b];
      if (N > 65537) continue;
      for (int c = 0; c < NSIZES; ++c) {
        const long R = SIZES[c];
        // K-slices: one of 1, 2, 4
        for (long nz : {1L, 2L, 8L, 256L}) {
          const int ks = gather_ks(R, gather_wgs(M, N, nz), sw);
          CHECK(ks == 1 || ks == 2 || ks == 4, "ks value", "M %ld N %ld R %ld ks %ld", M, N, R, (long)ks);
        }
        // split reduction, both kinds
        for (int kind = 1; kind <= 2; ++kind) {
          const int nz = split_r_chunks(M, N, R, kind, sw);
          CHECK(nz >= 1 && nz <= 8, "split count", "M %ld N %ld R %ld nz %ld", M, N, R, (long)nz);
          if (nz > 1) {
            const GatherChunks ch = split_r_plan(R, nz);
            CHECK(covers_once(R, ch), "split cover", "R %ld nz %ld chunk %ld final %ld", R, (long)nz, ch.r_chunk, (long)ch.nz);
            CHECK(ch.r_chunk % 32 == 0, "split chunk start", "R %ld chunk %ld", R, ch.r_chunk);
            CHECK(ch.nz <= nz, "split final nz", "R %ld planned %ld final %ld", R, (long)nz, (long)ch.nz);
            CHECK(gather_grid_ok(M, ch.nz), "split grid", "M %ld", M);
          }
        }
        // filter gradient: K = M rows of the output, Cout = N, reduction over R rows
        if (M <= 65537) {
          const long K = M, Cout = N, rows = R;
          {
            const int nz = wgrad_splits(K, Cout, rows, sw);
            const GatherChunks ch = wgrad_plan(rows, nz);
            CHECK(nz >= 1 && nz <= 256, "wgrad count", "K %ld Cout %ld M %ld nz %ld", K, Cout, rows, (long)nz);
            CHECK(covers_once(rows, ch) && ch.r_chunk % 16 == 0, "wgrad cover", "M %ld nz %ld chunk %ld final %ld", rows, (long)nz, ch.r_chunk, (long)ch.nz);
            CHECK(ch.nz <= nz, "wgrad final nz", "M %ld planned %ld final %ld", rows, (long)nz, (long)ch.nz);
            const size_t slab = gather_wgrad_slab_bytes(K, Cout, rows, sw), ws = gather_wgrad_ws_bytes(K, Cout, rows, sw);
            CHECK((size_t)ch.nz * K * Cout * sizeof(float) <= slab, "wgrad slabs fit", "K %ld Cout %ld M %ld", K, Cout, rows);
            const ColsumPlan p = colsum_plan(rows, (int)Cout, true);
            CHECK(slab + (size_t)p.nb * Cout * sizeof(float) <= ws, "wgrad partials fit", "K %ld Cout %ld M %ld nb %ld", K, Cout, rows, p.nb);
            // rcgan_deconv2d_bwd_weight: the tail for [rows2][cin] column sums at the end of a workspace of W .. W + 511 bytes
            for (long cin : {1L, 8L, 10L, 138L})
              for (long rows2 : {rows, 4 * rows}) {
                const size_t tail = colsum_tail_bytes(rows2, cin);
                const ColsumPlan q = colsum_plan(rows2, (int)cin, true);
                for (size_t extra : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)511}) {
                  const size_t W = ws + tail + extra, off = (W - tail) / 256 * 256;
                  CHECK(off >= slab && off + (size_t)q.nb * cin * sizeof(float) <= W, "deconv tail", "K %ld Cout %ld M %ld extra %ld", K, Cout, rows, (long)extra);
                }
              }
          }
          {
            const long m = R, k = M, n = N;
            const int nz = linear_wgrad_splits(m, k, n, sw);
            CHECK(m > 1024 || nz == 1, "linear direct rule", "m %ld nz %ld", m, (long)nz);
            const size_t slab = linear_wgrad_slab_bytes(m, k, n, sw), ws = linear_wgrad_plan_bytes(m, k, n, sw);
            if (nz > 1) {
              const GatherChunks ch = wgrad_plan(m, nz);
              CHECK(covers_once(m, ch) && ch.nz <= nz, "linear wgrad cover", "m %ld nz %ld chunk %ld final %ld", m, (long)nz, ch.r_chunk, (long)ch.nz);
              CHECK((size_t)ch.nz * k * n * sizeof(float) <= slab, "linear slabs fit", "m %ld k %ld n %ld", m, k, n);
            } else {
              CHECK(slab == 0, "linear direct has no slab", "m %ld k %ld n %ld", m, k, n);
            }
            const ColsumPlan p = colsum_plan(m, (int)n, true);
            CHECK(slab + (size_t)p.nb * n * sizeof(float) <= ws, "linear partials fit", "m %ld k %ld n %ld nb %ld", m, k, n, p.nb);
          }
        }
      }
      CHECK(gather_grid_ok(M, 1) == ((M + 63) / 64 <= 65535), "grid refusal", "M %ld", M);
    }
  CHECK(gather_grid_ok(65535L * 64, 4) && !gather_grid_ok(65535L * 64 + 1, 1) && !gather_grid_ok(64, 65536), "grid refusal", "limits %ld", 0L);
}

static void sweep_label_cols(const GatherSwitches& sw) {
  // rcgan_deconv2d_bwd_weight_concat: slabs | D | chunk partials | ... | column-sum tail
  for (long N : {1L, 8L, 9L, 33L, 256L})
    for (long hw : {7L, 14L, 28L, 32L})
      for (long cin : {1L, 64L, 128L})
        for (long c1 : {64L, 128L, 192L})
          for (long c2 : {1L, 10L, 16L})
            for (long k : {3L, 5L}) {
              const long K = k * k * cin, oh = (hw + 1) / 2, M = N * oh * oh, rows = N * hw * hw;
              const WgradColsLayout l = gather_wgrad_cols_layout(K, c1, c2, M, N, sw);
              const GatherChunks ch = wgrad_plan(M, wgrad_splits(K, c1, M, sw));
              CHECK((size_t)ch.nz * K * c1 <= l.D && l.D < l.partial && l.partial < l.end, "concat layout", "N %ld hw %ld cin %ld c1 %ld", N, hw, cin, c1);
              const size_t tail = colsum_tail_bytes(rows, cin), W = gather_wgrad_cols_ws_bytes(K, c1, c2, M, N, sw) + tail + 256;
              const ColsumPlan q = colsum_plan(rows, (int)cin, true);
              for (size_t extra : {(size_t)0, (size_t)100, (size_t)256}) {
                const size_t off = (W + extra - tail) / 256 * 256;
                CHECK(off >= l.end * sizeof(float) && off + (size_t)q.nb * cin * sizeof(float) <= W + extra, "concat tail", "N %ld hw %ld cin %ld c1 %ld", N, hw, cin, c1);
              }
            }
}

static void sweep_colsum() {
  for (int a = 0; a < NSIZES; ++a)
    for (int c = 1; c <= 520; ++c)
      for (int ws = 0; ws < 2; ++ws) {
        const long rows = SIZES[a];
        const ColsumPlan p = colsum_plan(rows, c, ws != 0);
        if (p.route == COLSUM_SINGLE) {
          // without a workspace always; with one only where neither partial route is on offer and the rows fit one pass
          const bool vec_ok = rows >= 2048 && c % 8 == 0 && c <= 256 && 256 % (c / 8) == 0, narrow_ok = rows >= 4096 && c <= 8;
          CHECK(p.nb == 0 && (!ws || (rows <= 4096 && !vec_ok && !narrow_ok)), "colsum single", "rows %ld c %ld ws %ld", rows, (long)c, (long)ws);
          continue;
        }
        CHECK(ws != 0, "colsum needs its workspace", "rows %ld c %ld", rows, (long)c);
        CHECK(p.nb >= 1 && p.nb * p.rows_per_blk >= rows && (p.nb - 1) * p.rows_per_blk < rows, "colsum cover", "rows %ld c %ld rpb %ld nb %ld", rows, (long)c, p.rows_per_blk, p.nb);
        CHECK((size_t)p.nb * c <= colsum_partial_floats(rows, c), "colsum partials fit", "rows %ld c %ld nb %ld", rows, (long)c, p.nb);
        if (p.route == COLSUM_VEC) {
          const int chunks = c / 8, nrl = 256 / chunks;
          CHECK(c % 8 == 0 && nrl * c == 2048 && chunks * nrl == 256, "colsum vec lanes", "rows %ld c %ld nrl %ld", rows, (long)c, (long)nrl);
          CHECK(p.nb <= 1024 && rows >= 2048, "colsum vec nb", "rows %ld c %ld nb %ld", rows, (long)c, p.nb);
        } else if (p.route == COLSUM_NARROW) {
          CHECK(c <= 8 && p.nb <= 1024 && rows >= 4096, "colsum narrow", "rows %ld c %ld nb %ld", rows, (long)c, p.nb);
        } else {
          CHECK(p.rows_per_blk == 2048 && rows > 4096, "colsum partial", "rows %ld c %ld", rows, (long)c);
        }
      }
}

static void sweep_s2(const GatherSwitches& sw) {
  for (int K = 1; K <= 5; ++K)
    for (int H = 1; H <= 9; ++H)
      for (int W = 1; W <= 9; ++W)
        for (int Cout : {1, 7, 32}) {
          int OH, OW, PT, PL;
          same_pad(H, K, 2, &OH, &PT);
          same_pad(W, K, 2, &OW, &PL);
          const S2Plan p = s2_classes(3, H, W, Cout, K, K, PT, PL, sw);
          long pixels = 0, taps = 0, maxM = 0, maxR = 0;
          // every pixel in one class; every tap (kh, kw) in the class of its parity: the classes' tap counts sum to K * K when all four exist
          for (int q = 0; q < p.ncls; ++q) {
            const S2Cls& c = p.tab.cls[q];
            pixels += c.M; taps += (long)c.nkh * c.nkw;
            if (c.M > maxM) maxM = c.M;
            if (c.R > maxR) maxR = c.R;
            CHECK(c.nkw >= 1 && c.dnkw.d == (unsigned)c.nkw && c.R == (long)c.nkh * c.nkw * Cout, "s2 class", "K %ld H %ld W %ld q %ld", (long)K, (long)H, (long)W, (long)q);
            CHECK(c.kh0 + 2 * (c.nkh - 1) < K && (c.nkh == 0 || c.kw0 + 2 * (c.nkw - 1) < K), "s2 taps inside", "K %ld H %ld W %ld q %ld", (long)K, (long)H, (long)W, (long)q);
            if (sw.s2_lpt && q > 0) CHECK(p.tab.cls[q - 1].R * p.tab.cls[q - 1].M >= c.R * c.M, "s2 order", "K %ld H %ld W %ld q %ld", (long)K, (long)H, (long)W, (long)q);
          }
          CHECK(p.ncls == (H > 1 ? 2 : 1) * (W > 1 ? 2 : 1), "s2 class count", "K %ld H %ld W %ld ncls %ld", (long)K, (long)H, (long)W, (long)p.ncls);
          CHECK(pixels == 3L * H * W && maxM == p.maxM && maxR == p.maxR, "s2 pixels", "K %ld H %ld W %ld pixels %ld", (long)K, (long)H, (long)W, pixels);
          if (p.ncls == 4) CHECK(taps == (long)K * K, "s2 taps", "K %ld H %ld W %ld taps %ld", (long)K, (long)H, (long)W, taps);
          for (long ncols : {1L, 2L, 3L, 4L, 5L})
            for (int mask = 0; mask < 2; ++mask)
              for (int f32 = 0; f32 < 2; ++f32) {
                const S2Route r = s2_route(f32, ncols, mask, Cout, 1024, p.maxR, sw);
                if (r == S2_TWO_STEP) CHECK(f32 && !mask && ncols <= 2 && Cout >= 32 && sw.narrow_two_step, "s2 two-step", "ncols %ld Cout %ld", ncols, (long)Cout);
                if (r == S2_NARROW) CHECK(ncols <= 4 && p.maxR > 0 && p.maxR * ncols * 4 <= S2_NARROW_MAX_LDS, "s2 narrow", "ncols %ld maxR %ld", ncols, p.maxR);
              }
        }
}

static void sweep_small() {
  // the K-group reduction area of gemm_gather_kernel ((KS - 1) x GG_RED_FLOATS, the kernel indexes it with that constant) inside the
  // KS x 4 operand buffers the launch allocates
  for (int ks : {1, 2, 4}) CHECK((long)(ks - 1) * GG_RED_FLOATS <= (long)ks * 4 * GG_XBUF, "ks reduction area", "ks %ld", (long)ks);
  CHECK(linear_tiny(65536, 4096) && !linear_tiny(65537, 4096) && !linear_tiny(65536, 4097), "linear_tiny", "%ld", 0L);
  CHECK(linear_skinny(1, 512, 16) && !linear_skinny(1, 511, 16) && !linear_skinny(1, 512, 17) && linear_skinny(65535, 512, 1) && !linear_skinny(65536, 512, 1), "linear_skinny", "%ld", 0L);
  for (long c = 1; c <= 12; ++c)
    for (size_t e : {(size_t)2, (size_t)4})
      for (uintptr_t a = 0; a < 8 * e; a += e) {      // base pointers offset by whole elements
        const int v = gather_vec_of(4096 + a, c, e);
        CHECK((v == 1 || v == 2 || v == 4) && c % v == 0 && (4096 + a) % (v * e) == 0, "vec_of", "c %ld a %ld e %ld v %ld", c, (long)a, (long)e, (long)v);
        CHECK(v == 4 || c % (2 * v) != 0 || (4096 + a) % (2 * v * e) != 0, "vec_of widest", "c %ld a %ld e %ld v %ld", c, (long)a, (long)e, (long)v);
      }
}

static int sweep() {
  struct Variant { const char* name; GatherSwitches sw; };
  std::vector<Variant> vs;
  vs.push_back({"default", GatherSwitches()});
  { GatherSwitches s; s.ks_force = 1; vs.push_back({"RCGAN_GG_KS=1", s}); }
  { GatherSwitches s; s.ks_force = 2; vs.push_back({"RCGAN_GG_KS=2", s}); }
  { GatherSwitches s; s.ks_min_steps = 1 << 30; vs.push_back({"RCGAN_GG_KS_MINSTEPS=off", s}); }
  { GatherSwitches s; s.ks2_min_wgs = 1L << 40; vs.push_back({"RCGAN_GG_KS2_MINWGS=off", s}); }
  { GatherSwitches s; s.split_r = 0; vs.push_back({"RCGAN_GG_SPLIT_R=0", s}); }
  { GatherSwitches s; s.wgrad_fit = 0; vs.push_back({"RCGAN_GG_WGRAD_FIT=0", s}); }
  { GatherSwitches s; s.narrow_two_step = 0; vs.push_back({"RCGAN_NARROW_TWO_STEP=0", s}); }
  { GatherSwitches s; s.s2_lpt = 0; vs.push_back({"RCGAN_S2_LPT=0", s}); }
  sweep_fastdiv();
  sweep_colsum();
  sweep_small();
  for (const Variant& v : vs) {
    const long before = g_checked;
    sweep_gemm(v.sw);
    sweep_label_cols(v.sw);
    sweep_s2(v.sw);
    printf("swept %s checks %ld\n", v.name, g_checked - before);
  }
  // the fit of wgrad_splits changes something, and only downwards
  {
    GatherSwitches off; off.wgrad_fit = 0;
    long changed = 0;
    for (long tiles_k = 1; tiles_k <= 64; ++tiles_k)
      for (long tiles_c = 1; tiles_c <= 8; ++tiles_c)
        for (long M : {1568L, 6272L, 65536L}) {
          const int a = wgrad_splits(tiles_k * 64, tiles_c * 64, M, GatherSwitches()), b = wgrad_splits(tiles_k * 64, tiles_c * 64, M, off);
          CHECK(a <= b && a >= 1, "wgrad fit only trims", "tiles %ld M %ld fit %ld plain %ld", tiles_k * tiles_c, M, (long)a, (long)b);
          changed += a != b;
        }
    CHECK(changed > 0, "wgrad fit reached", "%ld", changed);
  }
  long total = 0;
  for (const auto& kv : g_violations) { printf("violated %s x %ld\n", kv.first.c_str(), kv.second); total += kv.second; }
  printf("checked %ld violations %ld\n", g_checked, total);
  return total ? 1 : 0;
}

// ---- cases ----------------------------------------------------------------------------------------------------------------------
static const GatherSwitches DEF;

static std::string gemm_branch(long M, long N, long r_chunk, long nz) {
  char buf[96];
  if (!gather_grid_ok(M, nz)) return "refused";
  const int ks = gather_ks(r_chunk, gather_wgs(M, N, nz), DEF);
  const long steps = (r_chunk + 31) / 32;
  if (ks == 4) snprintf(buf, sizeof buf, "ks4/mod%ld", steps % 4);
  else if (ks == 2) snprintf(buf, sizeof buf, "ks2/%s", steps % 2 ? "odd" : "even");
  else snprintf(buf, sizeof buf, "ks1");
  return buf;
}
// a forward / dense data-gradient GEMM that may split its reduction (fp32 only)
static std::string split_or_gemm(bool f32, long M, long N, long R, int kind) {
  const int planned = f32 ? split_r_chunks(M, N, R, kind, DEF) : 1;
  if (planned <= 1) return "gemm/" + gemm_branch(M, N, R, 1);
  const GatherChunks ch = split_r_plan(R, planned);
  const long tiles = gp_cdiv(M, 64) * gp_cdiv(N, 64), steps = (R + 31) / 32;
  const char* cap = planned == 8 && 256 / tiles >= 8 && steps / 8 >= 8 ? "8" : (steps / 8 <= 256 / tiles ? "steps" : "tiles");
  const long last = R - (long)(ch.nz - 1) * ch.r_chunk;
  char buf[128];
  snprintf(buf, sizeof buf, "split/nz%d/cap_%s/last%ld/", ch.nz, cap, last);
  return buf + gemm_branch(M, N, ch.r_chunk, ch.nz);
}
static std::string linear_dgrad_branch(bool f32, long m, long k, long n) {
  if (linear_tiny(m * k, n)) return "tiny";
  return split_or_gemm(f32, m, k, n, 2);
}
static std::string colsum_branch(long rows, int c, bool ws) {
  const ColsumPlan p = colsum_plan(rows, c, ws);
  char buf[96];
  switch (p.route) {
    case COLSUM_SINGLE: return "single";
    case COLSUM_VEC: snprintf(buf, sizeof buf, "vec/rpb%ld/nb%ld/nrl%d", p.rows_per_blk, p.nb, 256 / (c / 8)); return buf;
    case COLSUM_NARROW: snprintf(buf, sizeof buf, "narrow/rpb%ld/nb%ld", p.rows_per_blk, p.nb); return buf;
    default: snprintf(buf, sizeof buf, "partial/nb%ld", p.nb); return buf;
  }
}
static std::string wgrad_branch(long K, long Cout, long M) {
  GatherSwitches plain; plain.wgrad_fit = 0;
  const int planned = wgrad_splits(K, Cout, M, DEF), unfit = wgrad_splits(K, Cout, M, plain);
  const GatherChunks ch = wgrad_plan(M, planned);
  const long tiles = gp_cdiv(K, 64) * gp_cdiv(Cout, 64), want = (1024 + tiles - 1) / tiles, maxs = (M + 255) / 256;
  const char* cap = planned != unfit ? "fit" : (unfit == 256 && want >= 256 && maxs >= 256 ? "256" : (maxs <= want ? "rows" : "tiles"));
  const long last = M - (long)(ch.nz - 1) * ch.r_chunk;
  char buf[160];
  snprintf(buf, sizeof buf, "slabs/planned%d/final%d/cap_%s/last%ld/", planned, ch.nz, cap, last);
  return buf + gemm_branch(K, Cout, ch.r_chunk, ch.nz);
}
struct Desc { int n, h, w, cin, cout, k, s, oh, ow, pt, pl; };
static std::string conv_fwd_branch(bool f32, const Desc& d, int ncols) {
  return split_or_gemm(f32, (long)d.n * d.oh * d.ow, ncols > 0 ? ncols : d.cout, (long)d.k * d.k * d.cin, 1);
}
static std::string conv_dgrad_branch(bool f32, const Desc& d, bool mask) {
  if (d.s != 2) return "gemm/" + gemm_branch((long)d.n * d.h * d.w, d.cin, (long)d.k * d.k * d.cout, 1);
  const S2Plan p = s2_classes(d.n, d.h, d.w, d.cout, d.k, d.k, d.pt, d.pl, DEF);
  const long m = (long)d.n * d.oh * d.ow, kcols = (long)d.k * d.k * d.cin;
  const S2Route r = s2_route(f32, d.cin, mask, d.cout, (size_t)m * kcols * sizeof(float), p.maxR, DEF);
  char buf[96];
  int zero = 0;
  for (int q = 0; q < p.ncls; ++q) zero += p.tab.cls[q].R == 0;
  snprintf(buf, sizeof buf, "/cls%d/zero%d", p.ncls, zero);
  if (r == S2_TWO_STEP) return "two_step/" + linear_dgrad_branch(true, m, kcols, d.cout);
  if (r == S2_NARROW) return "narrow/vec" + std::to_string(gather_vec_of(0, d.cout, 4)) + buf;
  return "s2gemm/" + gemm_branch(p.maxM, d.cin, p.maxR, p.ncls) + buf;
}

static int cases() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char kind[16], dt[16];
    long v[10] = {0};
    const int got = sscanf(line, "%15s %15s %ld %ld %ld %ld %ld %ld %ld %ld %ld", kind, dt, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8);
    if (got < 5) continue;
    const bool f32 = !strcmp(dt, "f32");
    std::string fwd = "-", dgrad = "-", wgrad, dbias, extra;
    if (!strcmp(kind, "linear")) {
      const long m = v[0], k = v[1], n = v[2];
      fwd = linear_skinny(m, k, n) ? "skinny" : linear_tiny(m * n, k) ? "tiny" : "gemm/" + gemm_branch(m, n, k, 1);
      dgrad = linear_dgrad_branch(f32, m, k, n);
      if (linear_tiny(k * n, m)) wgrad = "tiny";
      else {
        const int nz = linear_wgrad_splits(m, k, n, DEF);
        if (nz == 1) wgrad = "direct/" + gemm_branch(k, n, m, 1);
        else wgrad = wgrad_branch(k, n, m);
      }
      dbias = colsum_branch(m, (int)n, true);
    } else {
      Desc d = {(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], 0, 0, 0, 0};
      same_pad(d.h, d.k, d.s, &d.oh, &d.pt);
      same_pad(d.w, d.k, d.s, &d.ow, &d.pl);
      const long K = (long)d.k * d.k * d.cin, M = (long)d.n * d.oh * d.ow;
      if (!strcmp(kind, "concat")) {
        // v: n h w cin c1 c2 k s
        d.cout = (int)(v[4] + v[5]); d.k = (int)v[6]; d.s = (int)v[7];
        same_pad(d.h, d.k, d.s, &d.oh, &d.pt);
        same_pad(d.w, d.k, d.s, &d.ow, &d.pl);
        wgrad = wgrad_branch((long)d.k * d.k * d.cin, v[4], (long)d.n * d.oh * d.ow);
        dbias = colsum_branch((long)d.n * d.h * d.w, d.cin, true);
        extra = " chunks=" + std::to_string(gp_cdiv(d.n, WGRAD_LABEL_PER_CHUNK));
      } else if (!strcmp(kind, "conv")) {
        const size_t e = f32 ? 4 : 2;
        extra = " vec=x" + std::to_string(gather_vec_of(256 + v[8] * e, d.cin, e)) + "dy" + std::to_string(gather_vec_of(256 + v[8] * e, d.cout, e));
        fwd = conv_fwd_branch(f32, d, 0);
        dgrad = conv_dgrad_branch(f32, d, v[7] != 0);
        wgrad = wgrad_branch(K, d.cout, M);
        dbias = colsum_branch(M, d.cout, true);
      } else if (!strcmp(kind, "deconv")) {
        fwd = conv_dgrad_branch(f32, d, false);                     // rcgan_deconv2d_fwd = the data gradient of the descriptor
        dgrad = conv_fwd_branch(f32, d, (int)v[7]);                 // rcgan_deconv2d_bwd_data[_cols] = its forward
        wgrad = wgrad_branch(K, d.cout, M);
        dbias = colsum_branch((long)d.n * d.h * d.w, d.cin, v[8] != 0);      // (no tail: rcgan_deconv2d_bwd_weight passes no partials)
        extra = " tail=" + std::to_string(colsum_tail_bytes((long)d.n * d.h * d.w, d.cin));
      } else continue;
    }
    printf("case %s fwd=%s dgrad=%s wgrad=%s dbias=%s%s\n", kind, fwd.c_str(), dgrad.c_str(), wgrad.c_str(), dbias.c_str(), extra.c_str());
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "cases")) return cases();
  fprintf(stderr, "usage: %s sweep | cases < lines\n", argv[0]);
  return 2;
}
