// Stand-alone sweep of the batch-norm planner (csrc/bn_plan.h): host code only, nothing of HIP.  tests/test_bn_plan_cpu.py builds it
// with the host compiler and -fsanitize=address,undefined and runs it as a child process, once with RCGAN_BN_TREE_MIN set to the value
// of tests/conftest.py (the tree route on offer) and once without.
//
//   bn_plan_sweep sweep     every op x dtype x (un)labelled over the grid below, both workspace sizes; prints one line per violated
//                           invariant (the first MAX_SHOWN of each kind), the figures the GPU tests and the header take from here ("first_exceed", "first_refused",
//                           "halving"), a summary, and exits 1 if anything was violated
//   bn_plan_sweep cases     reads "op nseg n rows_per_sample c n_labels labelled dtype ws" lines (ws: huge | query) from standard input
//                           and prints route and sub-branch of each: what tests/test_gpu_bn_edges.py's case table claims
//
// The entry points of bn.hip are mirrored here (mirror_*): which shape they hand to bn_choose / bn_plan, and the one-segment calls the
// segmented ones fall back to.  The workspace query functions are RESTATED (query_bytes, query_bytes_labels), not linked: a GPU test
// pins the restatement to the library's values.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../robust-conditional-gan_amd/csrc/bn_plan.h"

// ---- rcgan_bn_workspace_bytes / rcgan_bn_workspace_bytes_labels, restated ----
static size_t query_bytes(long rows, long c) {
  long ng = (rows + 511) / 512 + 1;
  if (ng < 4096) ng = 4096;
  ng *= 2;
  return (size_t)(ng * 2 * c + 4 * c + 2 * 16 * c) * sizeof(float) + 256;
}
static size_t query_bytes_labels(long rows, long c, long n_labels) {
  const size_t base = query_bytes(rows, c);
  return n_labels > 16 ? base + (size_t)2 * (size_t)(n_labels - 16) * (size_t)c * sizeof(float) : base;
}

static const char* route_name(BnRoute r) {
  switch (r) { case BN_TREE: return "TREE"; case BN_COLUMN: return "COLUMN"; case BN_VEC: return "VEC"; case BN_SCALAR: return "SCALAR"; case BN_WIDE: return "WIDE"; }
  return "?";
}
static const char* op_name(BnOp o) {
  switch (o) { case BN_OP_STATS: return "STATS"; case BN_OP_STATS_SEG: return "STATS_SEG"; case BN_OP_APPLY: return "APPLY"; case BN_OP_APPLY_SEG: return "APPLY_SEG"; case BN_OP_BWD: return "BWD"; }
  return "?";
}
static bool op_from(const char* s, BnOp* o) {
  const BnOp all[] = {BN_OP_STATS, BN_OP_STATS_SEG, BN_OP_APPLY, BN_OP_APPLY_SEG, BN_OP_BWD};
  for (BnOp k : all) if (!strcmp(s, op_name(k))) { *o = k; return true; }
  return false;
}

// ---- violations ----
static const int MAX_SHOWN = 6;
static std::map<std::string, long> g_violations;
static long g_plans = 0;

static std::string shape_text(const BnShape& s) {
  char b[256];
  snprintf(b, sizeof b, "op=%s nseg=%d n=%d rps=%d c=%d n_labels=%d labelled=%d dtype=%d ws=%zu", op_name(s.op), s.nseg, s.n, s.rows_per_sample, s.c,
           s.n_labels, (int)s.labels, s.dtype, s.ws_bytes);
  return b;
}
static void violated(const char* what, const BnShape& s, const BnPlan& p, const char* detail = "") {
  long& k = g_violations[what];
  if (k++ < MAX_SHOWN)
    printf("VIOLATION %s: %s route=%s rpg=%ld ngroups=%d gps=%d nsub=%d wgs=%d need=%zu %s\n", what, shape_text(s).c_str(), route_name(p.route),
           p.rows_per_group, p.ngroups, p.groups_per_sample, p.nsub, p.workgroups, p.need, detail);
}
#define CHECK(cond, what) do { if (!(cond)) violated(what, s, p); } while (0)

struct Region { const char* name; size_t off, len; };

// the bytes a call may count on: what the header documents (times nseg for the segmented calls)
static size_t documented(const BnShape& s) { return (size_t)s.nseg * query_bytes_labels(s.rows(), s.c, s.n_labels); }

// Invariants of the reduction half of a plan (statistics, backward)
static void check_reduce(const BnShape& s, const BnPlan& p) {
  const long rows = s.rows();
  const bool bwd = s.op == BN_OP_BWD, labelled = bwd && s.labels;
  const size_t C = (size_t)s.c, nl = (size_t)s.n_labels, nseg = (size_t)s.nseg;
  // groups cover the rows, without an empty last one; 64-bit restatement of the int fields
  CHECK(p.rows_per_group >= 1 && p.ngroups >= 1 && p.nsub >= 1 && p.groups_per_sample >= 1, "positive geometry");
  CHECK(p.workgroups * p.nsub == p.ngroups, "workgroups * nsub == ngroups");
  CHECK((long)p.workgroups * p.rows_per_group >= rows, "groups cover the rows");
  CHECK(((long)p.workgroups - 1) * p.rows_per_group < rows, "no empty last group");
  if (labelled) {
    // never a group across two samples: whole samples to a workgroup, or whole groups to a sample
    if (p.nsub > 1) {
      CHECK(p.route == BN_COLUMN && p.rows_per_group == (long)p.nsub * s.rows_per_sample && p.rows_per_group == 32 && s.n % p.nsub == 0 && p.ngroups == s.n,
            "packed samples fill 32 rows");
    } else {
      CHECK(p.rows_per_group * p.groups_per_sample == s.rows_per_sample && (long)p.ngroups == (long)s.n * p.groups_per_sample, "groups never straddle a sample");
    }
    if (p.route == BN_TREE) CHECK(p.cluster_size == p.groups_per_sample && p.nclusters == s.n, "tree: one cluster per sample");
  } else {
    CHECK(p.nsub == 1, "nsub only with labels");
    const long rpg = p.rows_per_group;
    CHECK((long)p.ngroups == (rows + rpg - 1) / rpg, "ngroups fits in int");
  }
  // grid
  const unsigned gz = p.route == BN_COLUMN ? (unsigned)s.nseg : 1u;
  CHECK(p.grid_x >= 1 && p.grid_y >= 1 && p.grid_y <= 65535u && gz <= 65535u, "grid y, z <= 65535");
  switch (p.route) {
    case BN_TREE:
      CHECK(p.grid_x == (unsigned)p.ngroups && p.grid_y == (unsigned)s.nseg, "tree grid");
      CHECK(p.lds <= BN_TREE_MAX_LDS, "tree LDS");
      CHECK((size_t)p.nclusters * p.cluster_size >= (size_t)p.ngroups && ((size_t)p.nclusters - 1) * p.cluster_size < (size_t)p.ngroups, "clusters cover the groups");
      CHECK(nseg * ((size_t)p.nclusters + 1) <= BN_TREE_LINES, "tree counter lines");
      break;
    case BN_COLUMN:
      CHECK(p.grid_x == (unsigned)(s.c / 64) && p.grid_y == (unsigned)p.workgroups, "column grid");
      CHECK(p.lds <= 64 * 1024 && p.lds >= 2 * 32 * 64 * sizeof(float) && (!labelled || p.lds >= nl * 2 * 4 * 64 * sizeof(float)), "column LDS");
      if (s.op == BN_OP_STATS_SEG) CHECK(nseg * (C / 64) <= BN_SEG_LINES, "segment counter lines");
      else CHECK(nseg == 1 && C / 64 <= BN_COLUMN_LINES, "column counter lines");
      break;
    default:
      CHECK(p.grid_y == (unsigned)p.ngroups && (size_t)p.grid_x * (p.partial_vec ? 256 : 64) >= C, "partial grid");
      CHECK(nseg == 1, "partial kernels have no segments");
      break;
  }
  // workspace: the regions the route's kernels touch are disjoint and end at or before need
  std::vector<Region> rg;
  const size_t n_part = nseg * (size_t)p.ngroups * 2 * C;
  rg.push_back({"partial", p.partial, n_part});
  if (p.route == BN_TREE) {
    rg.push_back({"cpart", p.cpart, nseg * (size_t)p.nclusters * 2 * C});
    if (bwd) rg.push_back({"PQ", p.PQ, 2 * C});
  } else if (p.route == BN_COLUMN) {
    if (bwd) rg.push_back({"PQ", p.PQ, 2 * C});
  } else if (bwd) {
    rg.push_back({"s12", p.s12, 2 * C});
    if (p.route == BN_VEC) rg.push_back({"A", p.A, nl * C});
    if (p.route == BN_VEC || p.route == BN_WIDE) rg.push_back({"PQ", p.PQ, 2 * C});      // (the class kernel writes it on every wide call)
  }
  std::sort(rg.begin(), rg.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
  for (size_t k = 0; k < rg.size(); ++k) {
    if (k + 1 < rg.size() && rg[k].off + rg[k].len > rg[k + 1].off) {
      char d[96]; snprintf(d, sizeof d, "(%s [%zu, +%zu) into %s at %zu)", rg[k].name, rg[k].off, rg[k].len, rg[k + 1].name, rg[k + 1].off);
      violated("workspace regions disjoint", s, p, d);
    }
    if ((rg[k].off + rg[k].len) * sizeof(float) > p.need) {
      char d[96]; snprintf(d, sizeof d, "(%s ends at float %zu)", rg[k].name, rg[k].off + rg[k].len);
      violated("workspace regions end within need", s, p, d);
    }
  }
  // what the header promises (every n of the grid is <= 8192)
  if (s.n <= 8192) CHECK(p.need <= documented(s), "need <= documented query");
}

// Invariants of the apply half
static void check_apply(const BnShape& s, const BnPlan& p) {
  const long rows = s.rows();
  const bool fused = p.apply == BN_COLUMN;
  CHECK(p.apply == BN_COLUMN || p.apply == BN_VEC || p.apply == BN_SCALAR, "apply family");
  CHECK(!fused || bn_fused_ok(s.c), "fused apply only for fused channel counts");
  CHECK(p.apply != BN_VEC || s.c % 8 == 0, "vector apply only for c % 8 == 0");
  const long items = p.apply == BN_SCALAR ? rows * (long)s.c : rows * (long)s.c / 8;
  CHECK(p.apply_items == items && items >= 1, "apply_items");
  // the fused kernels index chunks with 32 bits (unsigned i += stride): items and one more stride must fit; the vector and scalar
  // kernels take a long
  if (fused) CHECK(items <= INT_MAX, "apply_items fits in int");
  CHECK(p.apply_grid >= 1 && p.apply_grid <= BN_APPLY_MAX_WGS && (long)p.apply_grid * 256 >= std::min(items, (long)BN_APPLY_MAX_WGS * 256), "apply grid");
  if (fused) CHECK(((long)p.apply_grid * 256) % (s.c / 8) == 0, "fused apply stride a multiple of the chunks per row");
  if (s.op == BN_OP_APPLY_SEG || s.op == BN_OP_STATS_SEG) CHECK(fused && s.nseg <= 65535, "segmented apply is the fused kernel");
  if (p.route == BN_VEC && s.op != BN_OP_STATS) {
    CHECK(p.need <= s.ws_bytes, "BN_VEC only where the tables fit");
    if (s.op == BN_OP_APPLY) {
      const size_t nlC = (size_t)s.n_labels * s.c;
      CHECK(p.A == 0 && p.B >= nlC && (p.B + nlC) * sizeof(float) <= p.need, "forward tables disjoint within need");
    }
  }
}

struct Seen { BnRoute stats, apply; bool per_segment; BnPlan plan; };

// ---- the entry points of bn.hip: the shapes they plan with ----
static void mirror(const BnShape& s, Seen* seen);

static void mirror_one(BnOp op, int n, int rps, int c, int nl, bool labels, int dtype, size_t ws, Seen* seen) {
  BnShape s = {op, 1, n, rps, c, nl, labels, dtype, ws};
  mirror(s, seen);
}

static void mirror(const BnShape& s, Seen* seen) {
  ++g_plans;
  const BnChoice ch = bn_choose(s);
  seen->per_segment = ch.per_segment;
  switch (s.op) {
    case BN_OP_STATS: {
      if (ch.route == BN_TREE) {          // rcgan_bn_stats: a call the tree takes must also hold what the column route would need
        const BnPlan p = bn_plan(s, BN_COLUMN);
        if (s.n <= 8192) CHECK(p.need <= documented(s), "need <= documented query");
      }
      const BnPlan p = bn_plan(s, ch.route);
      check_reduce(s, p);
      seen->stats = p.route; seen->plan = p;
      break;
    }
    case BN_OP_APPLY: {
      const BnPlan p = bn_plan(s, ch.route);
      check_apply(s, p);
      seen->apply = p.apply; seen->plan = p;
      break;
    }
    case BN_OP_STATS_SEG: case BN_OP_APPLY_SEG: {
      if (ch.per_segment) {               // bn_each_segment: rcgan_bn_stats(rows) and rcgan_bn_apply_fwd on each segment with the whole workspace
        Seen a = {}, b = {};
        if (s.op == BN_OP_STATS_SEG) mirror_one(BN_OP_STATS, 1, (int)s.rows(), s.c, 1, false, s.dtype, s.ws_bytes, &a);
        mirror_one(BN_OP_APPLY, s.n, s.rows_per_sample, s.c, s.n_labels, s.labels, s.dtype, s.ws_bytes, &b);
        seen->stats = a.stats; seen->apply = b.apply; seen->plan = s.op == BN_OP_STATS_SEG ? a.plan : b.plan;
        seen->plan.apply = b.apply; seen->plan.apply_grid = b.plan.apply_grid; seen->plan.apply_items = b.plan.apply_items;
      } else {
        const BnPlan p = bn_plan(s, ch.route);
        if (s.op == BN_OP_STATS_SEG) check_reduce(s, p);
        check_apply(s, p);
        seen->stats = p.route; seen->apply = p.apply; seen->plan = p;
      }
      break;
    }
    case BN_OP_BWD: {
      const BnPlan p = bn_plan(s, ch.route);
      check_reduce(s, p);
      check_apply(s, p);
      seen->stats = p.route; seen->apply = p.apply; seen->plan = p;
      break;
    }
  }
}

static bool index_ok(BnOp op, int nseg, long n, long rps, long c) {
  // bn_check_args: a segment's rows are an int, the tensor's element count a long; and what bn_index_ok adds
  const long rows = n * rps;
  if (rows > INT_MAX) return false;
  BnShape s = {op, nseg, op == BN_OP_STATS ? 1 : (int)n, op == BN_OP_STATS ? (int)rows : (int)rps, (int)c, 1, false, 0, 0};
  return bn_index_ok(s);
}

static int sweep() {
  const int N[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 130, 4096, 8000, 8001, 8192};
  const int RPS[] = {1, 2, 4, 8, 9, 16, 25, 32, 64, 256, 1024, 4096};
  const int CC[] = {1, 3, 8, 20, 24, 64, 72, 96, 128, 200, 256, 512, 1024, 2048, 4096};
  const int NL[] = {1, 2, 10, 16, 17, 100, 1024};
  const int NSEG[] = {1, 2, 8, 9, 256, 257};
  const BnOp OPS[] = {BN_OP_STATS, BN_OP_STATS_SEG, BN_OP_APPLY, BN_OP_APPLY_SEG, BN_OP_BWD};
  const size_t HUGE_WS = (size_t)1 << 46;
  long refused = 0;
  std::map<std::string, long> routes;
  for (BnOp op : OPS)
    for (int dtype : {RCGAN_F32, RCGAN_BF16})
      for (int lab = 0; lab < 2; ++lab)
        for (int n : N) for (int rps : RPS) for (int c : CC) for (int nl : NL) for (int nseg : NSEG) {
          const bool seg = op == BN_OP_STATS_SEG || op == BN_OP_APPLY_SEG;
          if (!seg && nseg != 1) continue;                       // the other calls have no segments
          if (op == BN_OP_STATS && (lab || nl != 1)) continue;   // rcgan_bn_stats has no labels
          if (!lab && nl != 1) continue;                         // refused by every entry point: n_labels > 1 needs labels
          if (!index_ok(op, nseg, n, rps, c)) { ++refused; continue; }
          for (int tight = 0; tight < 2; ++tight) {
            const long rows = (long)n * rps;
            BnShape s = {op, nseg, op == BN_OP_STATS ? 1 : n, op == BN_OP_STATS ? (int)rows : rps, c, nl, lab != 0, dtype, 0};
            s.ws_bytes = tight ? documented(s) : HUGE_WS;
            Seen seen = {};
            mirror(s, &seen);
            char key[64];
            snprintf(key, sizeof key, "%s/%s", op_name(op), seen.per_segment ? "per_segment" : route_name(seen.plan.route));
            ++routes[key];
          }
        }
  for (auto& kv : routes) printf("swept %s %ld\n", kv.first.c_str(), kv.second);
  printf("refused_by_index_check %ld\n", refused);

  // the smallest n at which a labelled backward needs more than the query function returns, per route (ws huge: the route of a caller
  // who has more), over channel counts on either side of every step of floor(32 / c)
  struct Probe { const char* name; int rps, c, nl; };
  const Probe probes[] = {{"COLUMN", 1, 64, 10}, {"COLUMN", 16, 64, 10}, {"COLUMN", 16, 2048, 16}, {"TREE", 16, 64, 10}, {"TREE", 64, 2048, 10},
                          {"VEC", 1, 24, 10}, {"VEC", 16, 200, 16}, {"VEC", 1, 8, 16}, {"VEC", 1, 40, 16}, {"VEC", 1, 32, 1},
                          {"SCALAR", 1, 20, 10}, {"SCALAR", 16, 3, 16}, {"SCALAR", 25, 20, 1}, {"SCALAR", 1, 100, 10}, {"SCALAR", 1, 33, 10},
                          {"SCALAR", 1, 31, 2}, {"SCALAR", 1, 17, 16}, {"SCALAR", 1, 16, 16}, {"SCALAR", 1, 1, 1},
                          {"WIDE", 1, 128, 17}, {"WIDE", 16, 20, 17}, {"WIDE", 16, 128, 1024}, {"WIDE", 1, 100, 100}};
  for (const Probe& pr : probes) {
    int first = 0;
    for (int n = 1; n <= 40000 && !first; ++n) {
      BnShape s = {BN_OP_BWD, 1, n, pr.rps, pr.c, pr.nl, true, RCGAN_BF16, HUGE_WS};
      const BnPlan p = bn_plan(s, bn_choose(s).route);
      if (strcmp(route_name(p.route), pr.name)) continue;
      if (p.need > documented(s)) first = n;
    }
    printf("first_exceed route=%s rps=%d c=%d n_labels=%d n=%d%s\n", pr.name, pr.rps, pr.c, pr.nl, first, first ? "" : " (never up to 40000, or the route is not on offer)");
  }
  // ... and what a caller who passes exactly the query's bytes meets: the first n at which the c % 8 == 0 route no longer holds its
  // tables (the call takes the scalar kernels), and the first n at which the call is refused, with the route that refuses
  const int QC[] = {1, 3, 16, 17, 20, 31, 32, 33, 100, 8, 24, 40, 200, 360, 64, 128, 2048};
  const int QK[] = {1, 10, 16, 17, 100, 1024};
  for (int c : QC) for (int nl : QK) for (int rps : {1, 16}) {
    int lost = 0, refused_at = 0; const char* by = "-";
    for (int n = 1; n <= 40000 && !refused_at; ++n) {
      BnShape s = {BN_OP_BWD, 1, n, rps, c, nl, true, RCGAN_BF16, 0};
      s.ws_bytes = documented(s);
      const BnPlan p = bn_plan(s, bn_choose(s).route);
      if (!lost && nl <= MAX_LABELS && c % 8 == 0 && !bn_fused_ok(c) && p.route != BN_VEC) lost = n;
      if (p.need > s.ws_bytes) { refused_at = n; by = route_name(p.route); }
    }
    printf("first_refused rps=%d c=%d n_labels=%d tables_lost=%d n=%d route=%s\n", rps, c, nl, lost, refused_at, by);
  }
  // rows at which the fp32 statistics change their rows per group (bn_group_rows): "halving c rows rpg_below rpg_at"
  for (int c : {20, 24, 64, 2048}) {
    long prev = -1;
    for (long rows = 1; rows <= 140000; ++rows) {
      BnShape s = {BN_OP_STATS, 1, 1, (int)rows, c, 1, false, RCGAN_F32, HUGE_WS};
      const BnChoice ch = bn_choose(s);
      if (ch.route == BN_TREE) break;
      const BnPlan p = bn_plan(s, ch.route);
      if (prev > 0 && p.rows_per_group != prev) printf("halving c=%d rows=%ld rpg_below=%ld rpg_at=%ld\n", c, rows, prev, p.rows_per_group);
      prev = p.rows_per_group;
    }
  }
  // is the chunks_per_row > 256 branch of bn_apply_grid reachable?  fused c <= BN_COLUMN_MAX_C
  printf("max_fused_chunks_per_row %d\n", BN_COLUMN_MAX_C / 8);

  long total = 0;
  for (auto& kv : g_violations) { printf("violated %ld x %s\n", kv.second, kv.first.c_str()); total += kv.second; }
  printf("plans %ld violations %ld tree_min %ld\n", g_plans, total, bn_switches().tree_min_elems);
  return total ? 1 : 0;
}

static int cases() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char opn[32], wsn[32];
    int nseg, n, rps, c, nl, lab, dtype;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %31s", opn, &nseg, &n, &rps, &c, &nl, &lab, &dtype, wsn) != 9) continue;
    BnOp op;
    if (!op_from(opn, &op)) { printf("error unknown op %s\n", opn); return 2; }
    const long rows = (long)n * rps;
    BnShape s = {op, nseg, op == BN_OP_STATS ? 1 : n, op == BN_OP_STATS ? (int)rows : rps, c, nl, lab != 0, dtype, 0};
    s.ws_bytes = !strcmp(wsn, "query") ? documented(s) : (size_t)1 << 46;
    Seen seen = {};
    mirror(s, &seen);
    const BnPlan& p = seen.plan;
    const bool reduces = op == BN_OP_STATS || op == BN_OP_STATS_SEG || op == BN_OP_BWD;
    const bool labelled = op == BN_OP_BWD && lab;
    const char* branch = "-";
    if (reduces && !seen.per_segment) {
      if (p.route == BN_WIDE) branch = p.partial_vec ? "wide_vec" : "wide_scalar";
      else if (!labelled) branch = "groups";
      else if (p.route == BN_COLUMN) branch = p.nsub > 1 ? "packed" : s.rows_per_sample < 32 ? "short" : p.groups_per_sample > 1 ? "split" : "sample";
      else if (p.route == BN_TREE) branch = p.groups_per_sample > 1 ? "split" : "sample";
      else branch = "sample";
    } else if (reduces) {
      branch = "groups";
    }
    const long per_stride = (long)p.apply_grid * 256;
    printf("case op=%s per_segment=%d route=%s branch=%s nsub=%d gps=%d rpg=%ld ngroups=%d workgroups=%d apply=%s apply_grid=%d apply_items=%ld strides=%ld need=%zu query=%zu\n",
           opn, (int)seen.per_segment, reduces ? route_name(seen.stats) : "-", branch, p.nsub, p.groups_per_sample, p.rows_per_group, p.ngroups, p.workgroups,
           op == BN_OP_STATS ? "-" : route_name(seen.apply), p.apply_grid, p.apply_items, op == BN_OP_STATS ? 0 : (p.apply_items + per_stride - 1) / per_stride,
           p.need, documented(s));
  }
  long total = 0;
  for (auto& kv : g_violations) total += kv.second;
  return total ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "cases")) return cases();
  fprintf(stderr, "usage: %s sweep | cases < lines\n", argv[0]);
  return 2;
}
