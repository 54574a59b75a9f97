// Which batch-norm kernels a call launches, and with what geometry: the one place that decides it (bn.hip launches what this says).
// Host-only and free of HIP: a pure function of the call's shape and of the environment switches below, so a stand-alone program can
// sweep it.
//
// route      kernels                                       taken when                                workspace (floats)                        launches fwd / bwd
// ---------  --------------------------------------------  ----------------------------------------  ----------------------------------------  ------------------
// BN_TREE    bn_tree_reduce_kernel, then the fused apply   c = 64 .. 2048, a power of two, and        partial [nseg][ng][2c] | cpart [nseg]      1 + 1 / 1 + 1
//            (two-level arrival tree: groups -> clusters   rows * c >= RCGAN_BN_TREE_MIN (off unless  [ncl][2c] | PQ [2c]
//            -> finisher; a workgroup streams whole rows)  set), counter lines for every cluster;
//                                                          labelled backward: label staging <= 96 KiB,
//                                                          groups + samples <= 8192 partial rows
// BN_COLUMN  bn_fused_reduce_kernel, bn_apply_fused_kernel c = 64 .. 2048, a power of two             partial [nseg][ng][2c] | (bwd) PQ [2c]     1 + 1 / 1 + 1
//            / bn_bwd_apply_fused_kernel (64-channel
//            column blocks, last arrival combines)
// BN_VEC     bn_partial_vec_kernel + finalize / combine,   c % 8 == 0; the apply (and with it the     fwd apply: A [nl][c] | B [nl][c]           2 + 2 / 2 + 2
//            bn_table_*_kernel + bn_*apply_vec_kernel      backward) only when ws_bytes holds the     bwd: partial [ng][2c] | s12 [2c] | A [nl]
//                                                          tables                                     [c] | PQ [2c]
// BN_SCALAR  bn_partial_kernel + finalize / combine,       everything else                            partial [ng][2c] | (bwd) s12 [2c]          2 + 1 / 2 + 1
//            bn_apply_fwd_kernel / bn_bwd_apply_kernel
// BN_WIDE    bn_sample_partial_kernel (c % 8 == 0, else    backward with n_labels > MAX_LABELS        partial [n][2c] | s12 [2c] | PQ [2c]       - / 2 + 1
//            bn_partial_kernel) + bn_bwd_class_kernel,     (17 .. BN_MAX_LABELS_WIDE): nothing scales
//            then the fused or the scalar backward apply   with the class count
//
// ng = row groups, ncl = clusters, nl = n_labels.  The statistics pass of a c % 8 == 0 tensor is BN_VEC whatever the workspace (it has
// no tables).  The forward apply has no tree: a tensor whose statistics took BN_TREE is applied by the fused kernel (BN_COLUMN).
// The segmented forward (rcgan_bn_fwd_segments) takes BN_TREE / BN_COLUMN with the segment as a grid dimension, or falls back to one
// segment at a time through the one-segment routes.
//
// Measured (scripts/bench_bn.py, MI355X): the reductions are bound by their serial arrival chain (write-through partials, drain,
// counter, finisher loads), not by the access pattern, and the tree has one hop more than the column kernel.  While the column
// kernel's arrival counters shared one 128-byte line the tree won on the biggest tensor ([320,32,32,256] bf16, 168 MB: statistics 37
// vs 55 us); with one counter per line the column kernel is faster at every size (that tensor: 36.2 vs 36.7 us, backward 202 vs 226
// us; [128,16,16,256]: 6.6 vs 16 us).  So the tree is OFF unless RCGAN_BN_TREE_MIN gives an element threshold; the tests lower the
// threshold so the path stays covered.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/rcgan_hip.h"

#define MAX_LABELS 16              // per-label accumulators in registers / LDS up to here
#define BN_MAX_LABELS_WIDE 1024    // ... per-sample partials in the workspace (BN_WIDE) up to here

// Limits that mirror the counter layout of common.h (bn.hip ties them to it with static_asserts)
#define BN_COLUMN_LINES 32                     // lines [RC_LCOUNTER_BN, RC_LCOUNTER_BNSEG): one per 64-channel column block
#define BN_COLUMN_MAX_C (64 * BN_COLUMN_LINES) // = 2048 channels
#define BN_SEG_LINES 256                       // lines [RC_LCOUNTER_BNSEG, + 256): one per (segment, column block)
#define BN_TREE_LINES 8192                     // tree_line_counters(): one per cluster + one per launch (and segment)
// ... and the tree kernel's own
#define BN_TREE_CLUSTER 16                     // groups per cluster (labelled backward: the groups of one sample instead)
#define BN_TREE_LABEL_STAGE_BYTES (96 * 1024)  // the finisher stages [n_labels][2c] floats per slice in LDS
#define BN_WS_PARTIAL_ROWS 8192                // partial rows [2c] that rcgan_bn_workspace_bytes counts at the least (2 x 4096)
#define BN_TREE_MAX_LDS (128 * 1024)
#define BN_APPLY_MAX_WGS 8192                  // grid-stride apply kernels

enum BnRoute { BN_TREE, BN_COLUMN, BN_VEC, BN_SCALAR, BN_WIDE };   // in order of precedence (BN_WIDE: its label count decides alone)

enum BnOp {
  BN_OP_STATS,       // rcgan_bn_stats
  BN_OP_STATS_SEG,   // the statistics half of rcgan_bn_fwd_segments
  BN_OP_APPLY,       // rcgan_bn_apply_fwd
  BN_OP_APPLY_SEG,   // rcgan_bn_apply_segments, and the apply half of rcgan_bn_fwd_segments
  BN_OP_BWD          // rcgan_bn_bwd / rcgan_bn_bwd2
};

struct BnShape {
  BnOp op;
  int nseg;                    // segments (1 outside the segmented calls)
  int n, rows_per_sample;      // samples (per segment) x rows; rcgan_bn_stats: 1 x rows
  int c, n_labels;
  bool labels;                 // conditional: the call has a label per sample
  int dtype;
  size_t ws_bytes;
  long rows() const { return (long)n * rows_per_sample; }
};

struct BnChoice {
  BnRoute route;               // meaningless when per_segment is set: plan nothing with it
  bool per_segment;            // segmented calls: one segment at a time through the one-segment entry points (which choose again)
};
#define BN_CHOICE_PER_SEGMENT BnChoice{BN_SCALAR, true}   // (the route is a filler)

struct BnPlan {
  BnRoute route;
  BnRoute apply;               // family of the apply kernel: BN_COLUMN (fused), BN_VEC (tables) or BN_SCALAR
  bool partial_vec;            // partial + finish routes: the 8-wide partial kernel
  long rows_per_group;
  int ngroups;                 // partial rows in the workspace (per segment)
  int groups_per_sample;       // labelled backward: a sample's groups (tree: = cluster_size)
  int nsub;                    // column route, samples of < 32 rows: samples per workgroup
  int workgroups;              // ngroups / nsub
  int cluster_size, nclusters; // tree
  unsigned grid_x, grid_y;     // reduction (or partial) grid; z = nseg
  size_t lds;                  // dynamic LDS of the reduction
  long apply_items;            // 8-element chunks (fused, vec) or elements (scalar) of one segment
  int apply_grid;
  size_t partial, cpart, s12, A, B, PQ;   // workspace layout: offsets in floats
  size_t need;                 // bytes
};

// The environment switches, each parsed here and nowhere else, once, at the first call that plans.
struct BnSwitches {
  long tree_min_elems;         // RCGAN_BN_TREE_MIN (elements; RCGAN_BN_TREE=0 or unset: never)
  long tree_groups;            // RCGAN_BN_TREE_GROUPS: workgroups the tree aims at
  long bwd_wgs, bwd_maxg;      // RCGAN_BN_BWD_WGS / RCGAN_BN_BWD_MAXG: workgroups aimed at / most groups of the labelled column backward
};
static inline const BnSwitches& bn_switches() {
  static const BnSwitches s = [] {
    BnSwitches v;
    const char* e = getenv("RCGAN_BN_TREE");
    const char* m = getenv("RCGAN_BN_TREE_MIN");
    v.tree_min_elems = (e && atoi(e) == 0) ? (1L << 62) : (m ? atol(m) : (1L << 62));
    const char* g = getenv("RCGAN_BN_TREE_GROUPS");
    v.tree_groups = g ? atol(g) : 512;
    // (round 3, same box: 512 / 512 -> 5.827 ms per iteration, 1024 / 1024 -> 5.801, 2048 / 2048 -> 5.815: the 32 x 32 layers gain from more
    // workgroups, the 8 x 8 / 16 x 16 ones lose to the longer finisher)
    const char* w = getenv("RCGAN_BN_BWD_WGS");
    v.bwd_wgs = w ? atol(w) : 1024;
    const char* x = getenv("RCGAN_BN_BWD_MAXG");
    v.bwd_maxg = x ? atol(x) : 1024;
    return v;
  }();
  return s;
}

static inline long bn_cdiv(long a, long b) { return (a + b - 1) / b; }

// fused kernels: 64-channel column blocks, thread-fixed channel chunks in the apply kernels
static inline bool bn_fused_ok(int c) {
  return c >= 64 && c <= BN_COLUMN_MAX_C && (c & (c - 1)) == 0;      // power of two: chunks per row divide (or are) the block size
}
// tree: power-of-two channel counts (full rows per workgroup need c/8 <= 256 chunk lanes), from the switch's size on
static inline bool bn_tree_ok(long rows, int c) { return bn_fused_ok(c) && rows * (long)c >= bn_switches().tree_min_elems; }

static BnPlan bn_plan(const BnShape& s, BnRoute route);

// The route of a call.  Everything that decides between kernel families is here.
static inline BnChoice bn_choose(const BnShape& s) {
  const bool fused = bn_fused_ok(s.c);
  // segmented forward: channel counts without fused kernels, or more (segment, column block) pairs than counter lines
  if (s.op == BN_OP_STATS_SEG && (!fused || (long)s.nseg * (s.c / 64) > BN_SEG_LINES)) return BN_CHOICE_PER_SEGMENT;
  // segmented apply: one segment is the plain apply; the vector and scalar apply kernels have no segment dimension
  if (s.op == BN_OP_APPLY_SEG && (s.nseg == 1 || !fused)) return BN_CHOICE_PER_SEGMENT;
  const bool reduces = s.op == BN_OP_STATS || s.op == BN_OP_STATS_SEG || s.op == BN_OP_BWD;
  if (s.op == BN_OP_BWD && s.n_labels > MAX_LABELS) return {BN_WIDE, false};
  if (reduces && bn_tree_ok(s.rows(), s.c)) {
    const bool labelled = s.op == BN_OP_BWD && s.labels;
    const BnPlan t = bn_plan(s, BN_TREE);
    // one counter line per cluster and one per launch, for every segment; with labels a cluster is a sample, and the group and
    // cluster partials together stay within the partial rows the workspace query counts
    const bool fits = (long)s.nseg * (t.nclusters + 1L) <= BN_TREE_LINES && (!labelled || (long)t.ngroups + t.nclusters <= BN_WS_PARTIAL_ROWS);
    if (fits && (!labelled || (size_t)s.n_labels * 2 * s.c * sizeof(float) <= BN_TREE_LABEL_STAGE_BYTES)) return {BN_TREE, false};
  }
  if (fused) return {BN_COLUMN, false};
  // 8-wide kernels; their apply needs room for the affine tables (the statistics pass has none)
  if (s.c % 8 == 0 && (s.op == BN_OP_STATS || bn_plan(s, BN_VEC).need <= s.ws_bytes)) return {BN_VEC, false};
  return {BN_SCALAR, false};
}

// rows per group of the column / partial kernels
static inline long bn_group_rows(long rows, int c, int dtype) {
  long g = 512;
  while (rows / g > 2048) g *= 2;
  // fp32 path (MNIST: 64-channel critic layers of 1024 .. 25088 rows): 512 rows per workgroup are 128 dependent rounds of loads in 2 .. 49
  // workgroups -- a latency chain of 17-20 us for a few hundred KB.  Shorter groups until ~256 workgroups exist (the finisher reads <= 256 partials)
  if (dtype == RCGAN_F32 && c > 0)
    while (g > 32 && (rows / g) * (c / 64 > 0 ? c / 64 : 1) < 256) g /= 2;
  return g;
}

// fused apply: the stride (b * 256) must be a multiple of the chunks per row.  It always is: bn_fused_ok admits powers of two up to
// BN_COLUMN_MAX_C = 2048 channels, so the chunks per row are a power of two <= 256 (tests/tools/bn_plan_sweep.cpp checks every plan)
static_assert(BN_COLUMN_MAX_C / 8 <= 256, "chunks per row of the fused apply divide the 256 threads of a workgroup");
static inline int bn_apply_grid(long items) {
  long b = (items + 255) / 256;
  if (b > BN_APPLY_MAX_WGS) b = BN_APPLY_MAX_WGS;
  if (b < 1) b = 1;
  return (int)b;
}

// What the index types take: a segment's rows are an int in the kernels' arguments, element offsets 64-bit; the fused apply kernels
// count a segment's 8-element chunks in 32 bits (the statistics call applies nothing)
static inline bool bn_index_ok(const BnShape& s) {
  const long rows = s.rows();
  if (rows > INT32_MAX || s.nseg > INT64_MAX / (rows * s.c)) return false;
  return s.op == BN_OP_STATS || !bn_fused_ok(s.c) || rows * s.c / 8 <= INT32_MAX;
}

// Geometry, workspace layout and need of `route` for the call `s`.
static inline BnPlan bn_plan(const BnShape& s, BnRoute route) {
  BnPlan p = {};
  const long rows = s.rows();
  const int c = s.c;
  const size_t C = (size_t)c, nl = (size_t)s.n_labels, nseg = (size_t)s.nseg;
  const bool bwd = s.op == BN_OP_BWD, labelled = bwd && s.labels;
  const bool reduces = bwd || s.op == BN_OP_STATS || s.op == BN_OP_STATS_SEG;
  p.route = route;
  p.groups_per_sample = 1; p.nsub = 1; p.cluster_size = BN_TREE_CLUSTER;

  if (reduces) {
    // ---- row groups ----
    if (route == BN_TREE) {
      const int RL = 256 / (c / 8) > 0 ? 256 / (c / 8) : 1;       // row lanes
      const long target = bn_switches().tree_groups;
      if (labelled) {
        // with labels a cluster is exactly one sample, split into gps groups of whole row-lane rounds and at least 16 rows
        long rpg = s.rows_per_sample;
        int gps = 1;
        while ((long)s.n * gps < target && rpg % 2 == 0 && rpg / 2 >= 16 && (rpg / 2) % RL == 0 && gps < 16) { gps *= 2; rpg /= 2; }
        p.rows_per_group = rpg; p.ngroups = s.n * gps; p.cluster_size = gps;
      } else {
        // ~target workgroups, a multiple of the row lanes, at least 16 rows
        long rpg = bn_cdiv(rows, target);
        if (rpg < 16) rpg = 16;
        p.rows_per_group = (rpg + RL - 1) / RL * RL;
        p.ngroups = (int)bn_cdiv(rows, p.rows_per_group);
      }
      p.groups_per_sample = p.cluster_size;
      p.nclusters = (int)bn_cdiv(p.ngroups, p.cluster_size);
    } else if (labelled && route == BN_COLUMN) {
      // groups never straddle samples; split each sample until the grid has enough workgroups (six fit on a CU); samples of
      // fewer than 32 rows (the 4x4 stage) go nsub to a workgroup, which still writes one partial row per sample
      const BnSwitches& sw = bn_switches();
      const int rps = s.rows_per_sample;
      long rpg = rps;
      int gps = 1;
      if (rps < 32 && 32 % rps == 0 && s.n % (32 / rps) == 0) { p.nsub = 32 / rps; rpg = 32; }
      else while ((long)s.n * gps * (c / 64) < sw.bwd_wgs && rpg % 2 == 0 && rpg / 2 >= 32 && (long)s.n * gps * 2 <= sw.bwd_maxg) { gps *= 2; rpg /= 2; }
      p.rows_per_group = rpg; p.groups_per_sample = gps; p.ngroups = s.n * gps;
    } else if (labelled) {
      p.rows_per_group = s.rows_per_sample; p.ngroups = s.n;        // one group per sample: group label = sample label
    } else {
      // kept difference: the segmented forward groups without the fp32 refinement rcgan_bn_stats and the backward apply
      p.rows_per_group = s.op == BN_OP_STATS_SEG ? bn_group_rows(rows, 0, -1) : bn_group_rows(rows, c, s.dtype);
      p.ngroups = (int)bn_cdiv(rows, p.rows_per_group);
    }
    p.workgroups = p.ngroups / p.nsub;

    // ---- grid, LDS, workspace ----
    const size_t n_part = nseg * (size_t)p.ngroups * 2 * C;
    switch (route) {
      case BN_TREE: {
        p.grid_x = (unsigned)p.ngroups; p.grid_y = (unsigned)s.nseg;
        const int Q = 2 * c / 4, SL = Q >= 256 ? 1 : 256 / Q;
        p.lds = 16384;                                              // [2][RL][c] floats = 4096 floats
        if (4 * C * sizeof(float) > p.lds) p.lds = 4 * C * sizeof(float);
        if (labelled) { const size_t l2 = (size_t)SL * nl * 2 * C * sizeof(float); if (l2 > p.lds) p.lds = l2; }
        p.cpart = n_part;
        p.PQ = p.cpart + nseg * (size_t)p.nclusters * 2 * C;
        p.need = (p.PQ + 2 * C) * sizeof(float);
        break;
      }
      case BN_COLUMN: {
        p.grid_x = (unsigned)(c / 64); p.grid_y = (unsigned)p.workgroups;
        // the row buffer red[2][32][64]; the labelled backward's finisher reuses it as lacc[2][n_labels][4][64]
        const size_t red = 2 * 32 * 64 * sizeof(float), lacc = labelled ? nl * 2 * 4 * 64 * sizeof(float) : 0;
        p.lds = red > lacc ? red : lacc;
        p.PQ = n_part;
        p.need = (n_part + (bwd ? 2 * C : 0)) * sizeof(float);
        break;
      }
      case BN_VEC: case BN_SCALAR: case BN_WIDE:
        p.partial_vec = route == BN_VEC || (route == BN_WIDE && c % 8 == 0);
        p.grid_x = (unsigned)(p.partial_vec ? bn_cdiv(c / 8, 32) : bn_cdiv(c, 64)); p.grid_y = (unsigned)p.ngroups;
        p.s12 = n_part;
        if (route == BN_VEC) { p.A = p.s12 + 2 * C; p.PQ = p.A + nl * C; }
        else p.PQ = p.s12 + 2 * C;
        p.need = (!bwd ? n_part : route == BN_SCALAR ? p.s12 + 2 * C : p.PQ + 2 * C) * sizeof(float);
        break;
    }
  }

  // ---- apply ----
  if (!reduces) {
    p.apply = route;
    if (route == BN_VEC) { p.B = nl * C; p.need = 2 * nl * C * sizeof(float); }      // A [nl][c] | B [nl][c]
  } else if (route == BN_VEC || route == BN_SCALAR) {
    p.apply = route;
  } else {
    p.apply = bn_fused_ok(c) ? BN_COLUMN : BN_SCALAR;                                  // (BN_WIDE takes any channel count)
  }
  p.apply_items = p.apply == BN_SCALAR ? rows * c : rows * c / 8;
  p.apply_grid = bn_apply_grid(p.apply_items);
  return p;
}
