"""The fp32 gather GEMM family of csrc/conv_direct.hip at every branch of its launch plan (csrc/gather_plan.h), through the C ABI, against
float64 references, inside guard bands (tests/guard.py).

Every case names, in its table, the branch each of its four calls (forward, data gradient, filter gradient, bias gradient) takes;
tests/test_gather_plan_cpu.py feeds the tables to tests/tools/gather_plan_sweep.cpp and asserts that each case lands there and that the
tables together reach every entry of BRANCHES.  The switches of the planner are read once per process, so the branches are reached by
shape alone.

Two passes per case:
  exact     inputs are integers in [-3, 3], filters integers in [-2, 2], sigma = 0.5, accumulate targets pre-filled with integers.  The
            reference of |inputs| bounds every partial sum below 2^24 (asserted on the host first), so every fp32 partial sum is exact
            whatever the split, slice count or summation order, and on the split-bf16 ("high") route too (the integers have a zero lo
            part): every fp32 output must EQUAL the float64 reference, every 16-bit output half_round(mode, reference).  A dropped or
            doubled K-step, row, slab or chunk is an integer difference.
  gaussian  only where no reduction of the case exceeds 8192 terms: inputs and sigma = 1.7 as in test_gpu_ops.test_conv2d_fwd_bwd,
            tolerances of that file (TOL[mode] forward and data gradient, 2e-4 filter and bias gradient).  Catches a wrong 1/sigma or bias.

Workspaces: production-like (64 MiB between guard margins), then exactly what the op's query returns; the transposed convolutions also
with the query plus the column-sum tail.  After every pass: Guard.check(), no output element left unwritten.

Contexts: fp32 at "highest" and "high" matmul precision for every case; bf16 and fp16 for the cases marked h16.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import nn
from tests.guard import guarded
from tests.gpu_util import assert_close, half_round, make_ctx
from tests.test_gpu_ops import TOL

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- case tables
# conv: rcgan_conv2d_fwd / _bwd_data / _bwd_weight with RCGAN_CONV_FORCE_DIRECT on the descriptor (n, h, w, cin, cout, k, stride).
#   mask: RCGAN_CONV_IN_RELU (ReLU on the forward input, mask on the data gradient); off: base pointers of x and dy offset by that many
#   elements; h16: also on the 16-bit contexts.  claims: what gather_plan_sweep prints for the call: a prefix, or "prefix*suffix".
CONV_CASES = {
    # K-slices: 1 (< 8 K-steps); 4 with steps % 4 = 0, 1, 2, 3 on one or two tiles (M = 98: a tail tile; N = 33, 10: dead quadrants)
    "ks1 3x3 c8": dict(d=(2, 5, 5, 8, 10, 3, 1), h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1", wgrad="slabs/planned1/final1/cap_rows", dbias="single")),
    "ks1 3x3 c20": dict(d=(2, 5, 5, 20, 9, 3, 1), h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1")),
    "ks4 mod0 5x5 c9": dict(d=(2, 7, 7, 9, 33, 5, 1), h16=True, claims=dict(fwd="gemm/ks4/mod0", dgrad="gemm/ks4/mod2")),
    "ks4 mod1 3x3 c32": dict(d=(2, 7, 7, 32, 33, 3, 1), claims=dict(fwd="gemm/ks4/mod1", dgrad="gemm/ks4/mod2")),
    "ks4 mod2 3x3 c33": dict(d=(1, 13, 5, 33, 10, 3, 1), mask=1, claims=dict(fwd="gemm/ks4/mod2", dgrad="gemm/ks1")),
    "ks4 mod3 5x5 c13": dict(d=(2, 7, 7, 13, 20, 5, 1), claims=dict(fwd="gemm/ks4/mod3", dgrad="gemm/ks4/mod0")),
    "ks4 mod0 3x3 c40": dict(d=(1, 5, 13, 40, 37, 3, 1), claims=dict(fwd="gemm/ks4/mod0", dgrad="gemm/ks4/mod3")),
    "ks4 dgrad mod1 c29": dict(d=(1, 9, 9, 12, 29, 3, 1), claims=dict(fwd="gemm/ks1", dgrad="gemm/ks4/mod1")),
    # 16 x 16 output tiles: two K-slices, even and odd step counts; the filter gradient's split count capped by ceil(M / 256)
    "ks2 even 5x5 c12": dict(d=(16, 32, 32, 12, 64, 5, 1), h16=True,
                             claims=dict(fwd="gemm/ks2/even", dgrad="gemm/ks2/even", wgrad="slabs/planned64/final64/cap_rows", dbias="vec/rpb256/nb64/nrl32")),
    "ks2 odd 5x5 c13": dict(d=(16, 32, 32, 13, 64, 5, 1), claims=dict(fwd="gemm/ks2/odd", dgrad="gemm/ks2/even", wgrad="slabs/planned64*/ks2/even")),
    "ks2 dgrad odd c13": dict(d=(16, 32, 32, 12, 13, 5, 1), claims=dict(fwd="gemm/ks2/even", dgrad="gemm/ks2/odd")),
    # misaligned base pointers with c % 4 == 0: vec_of falls to 1 and 2
    "offset 0": dict(d=(2, 7, 7, 12, 20, 3, 1), h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1", vec="x4dy4")),
    "offset 1": dict(d=(2, 7, 7, 12, 20, 3, 1), off=1, h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1", vec="x1dy1")),
    "offset 2": dict(d=(2, 7, 7, 12, 20, 3, 1), off=2, h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1", vec="x2dy2")),
    # scalar channel counts
    "scalar c1": dict(d=(3, 6, 5, 1, 3, 5, 1), h16=True, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1")),
    "scalar c3 c7": dict(d=(3, 6, 5, 3, 7, 3, 1), mask=1, claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1")),
    "scalar c7 c1": dict(d=(2, 6, 6, 7, 1, 5, 1), claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1")),
    # the grid limit: 65535 row tiles run; the bias gradient's narrow route doubles its rows per block twice; 256 splits of the filter gradient
    "grid limit": dict(d=(255, 257, 64, 1, 1, 1, 1), claims=dict(fwd="gemm/ks1", dgrad="gemm/ks1", wgrad="slabs/planned256/final256/cap_256", dbias="narrow/rpb4096/nb1024")),
    "narrow doubling": dict(d=(17, 61681, 1, 1, 1, 1, 1), h16=True, claims=dict(dbias="narrow/rpb2048/nb513", wgrad="slabs/planned256/final256/cap_256")),
    # stride-2 data gradients on the GEMM: 5x5 (4 / 6 / 6 / 9 taps) with odd sizes, 3x3, 1x1 (three classes without a tap), H = 1 (two classes)
    "s2 5x5 odd": dict(d=(3, 7, 5, 10, 12, 5, 2), mask=1, h16=True, claims=dict(dgrad="s2gemm/ks1/cls4/zero0")),
    "s2 5x5 ks4": dict(d=(3, 7, 5, 9, 33, 5, 2), claims=dict(dgrad="s2gemm/ks4/mod2/cls4/zero0")),
    "s2 3x3": dict(d=(2, 6, 6, 7, 20, 3, 2), h16=True, claims=dict(dgrad="s2gemm/ks1/cls4/zero0")),
    "s2 1x1": dict(d=(2, 5, 5, 8, 16, 1, 2), h16=True, claims=dict(dgrad="s2gemm/ks1/cls4/zero3")),
    "s2 h1": dict(d=(3, 1, 6, 5, 9, 5, 2), claims=dict(dgrad="s2gemm/ks1/cls2/zero0")),
    "s2 w1": dict(d=(3, 6, 1, 5, 9, 3, 2), mask=1, claims=dict(dgrad="s2gemm/ks1/cls2/zero0")),
    # narrow stride-2 routes: two-step (fp32, <= 2 columns, cout >= 32, no mask), the 16-lanes-per-pixel kernel at VEC 4 / 2 / 1 and
    # N = 3, 4, the GEMM once the filter slice passes 48 KiB
    "two-step": dict(d=(3, 7, 7, 1, 64, 5, 2), claims=dict(dgrad="two_step/tiny")),
    "two-step 2 cols odd": dict(d=(2, 9, 5, 2, 32, 5, 2), claims=dict(dgrad="two_step/tiny")),
    "two-step h16 is narrow": dict(d=(3, 7, 7, 1, 64, 5, 2), h16=True, only16=True, claims=dict(dgrad="narrow/vec4/cls4/zero0")),
    "narrow cout31": dict(d=(3, 7, 7, 1, 31, 5, 2), h16=True, claims=dict(dgrad="narrow/vec1/cls4/zero0")),
    "narrow mask vec4": dict(d=(3, 7, 5, 2, 64, 5, 2), mask=1, claims=dict(dgrad="narrow/vec4/cls4/zero0")),
    "narrow vec2 n3": dict(d=(2, 6, 6, 3, 34, 3, 2), claims=dict(dgrad="narrow/vec2/cls4/zero0")),
    "narrow n4 1x1": dict(d=(2, 5, 5, 4, 8, 1, 2), h16=True, claims=dict(dgrad="narrow/vec4/cls4/zero3")),
    "n4 past 48k": dict(d=(2, 6, 6, 4, 342, 5, 2), claims=dict(dgrad="s2gemm/ks4/mod1/cls4/zero0")),
    # split reduction of the forward: thresholds R = 992 / 993 and 127 / 128 tiles; the count capped by steps / 8, by 256 / tiles, by 8
    "split off r992": dict(d=(1, 8, 8, 992, 16, 1, 1), h16=True, claims=dict(fwd="gemm/ks4/mod3")),
    "split on r993": dict(d=(1, 8, 8, 993, 16, 1, 1), h16=True, claims=dict(fwd="split/nz4/cap_steps/last225/ks4/mod0")),
    "split 127 tiles": dict(d=(127, 8, 8, 993, 16, 1, 1), claims=dict(fwd="split/nz2/cap_tiles/last481/ks4/mod0")),
    "split off 128 tiles": dict(d=(128, 8, 8, 993, 16, 1, 1), claims=dict(fwd="gemm/ks4/mod0")),
    "split cap 8": dict(d=(1, 4, 4, 2100, 16, 1, 1), claims=dict(fwd="split/nz8/cap_8/last")),
    "split 5x5": dict(d=(2, 4, 4, 64, 70, 5, 2), claims=dict(fwd="split/nz6/cap_steps", dgrad="s2gemm/ks4")),
    # filter gradient: slab counts 2, 3, 17 with K * Cout no multiple of 64; a last chunk of 10 rows; 256 planned, 241 used
    "wgrad nz2": dict(d=(3, 10, 10, 3, 7, 3, 1), claims=dict(wgrad="slabs/planned2/final2/cap_rows")),
    "wgrad nz3": dict(d=(6, 10, 10, 3, 7, 3, 1), h16=True, claims=dict(wgrad="slabs/planned3/final3/cap_rows")),
    "wgrad nz17": dict(d=(17, 16, 16, 3, 7, 3, 1), claims=dict(wgrad="slabs/planned17/final17/cap_rows", dbias="narrow/rpb1024/nb5")),
    "wgrad last 10 rows": dict(d=(14, 25, 11, 3, 7, 3, 1), claims=dict(wgrad="slabs/planned16/final16/cap_rows/last10/")),
    "wgrad 241 of 256": dict(d=(65537, 1, 1, 3, 7, 1, 1), claims=dict(wgrad="slabs/planned256/final241/cap_256/last257/")),
    "wgrad cap tiles": dict(d=(5, 32, 32, 512, 512, 1, 1), claims=dict(wgrad="slabs/planned16/final16/cap_tiles", fwd="gemm/ks2/even", dbias="partial/nb3")),
}

# deconv: rcgan_deconv2d_fwd / _bwd_data_cols / _bwd_weight on the descriptor (n, h, w, cin, cout, k, stride) of the convolution it
#   transposes (input [n, oh, ow, cout], output [n, h, w, cin]).  ncols: only the first ncols input channels get a gradient.
DECONV_CASES = {
    "deconv 5x5": dict(d=(3, 14, 14, 6, 10, 5, 2), h16=True, claims=dict(fwd="s2gemm/ks1/cls4/zero0", dgrad="gemm/ks1", dbias="single")),
    # two-step with bias and odd sizes whose inner dense data gradient splits its reduction
    "two-step split": dict(d=(11, 31, 31, 1, 1024, 5, 2), claims=dict(fwd="two_step/split/nz4/cap_steps")),
    # the generator's 7x7x138 -> 14x14x128 layer at n = 32: 150 tiles, M = 1568, 7 -> 6 splits (whole rounds); at n = 24 the rows cap at 5
    "fit 7 to 6": dict(d=(32, 14, 14, 128, 138, 5, 2), ncols=128, h16=True,
                       claims=dict(wgrad="slabs/planned6/final6/cap_fit*/ks2/odd", dgrad="split/nz5/cap_tiles", dbias="vec/rpb256/nb25/nrl16")),
    "fit missed": dict(d=(24, 14, 14, 128, 138, 5, 2), ncols=128, claims=dict(wgrad="slabs/planned5/final5/cap_rows", dbias="vec/rpb256/nb19/nrl16")),
    # rcgan_deconv2d_bwd_data_cols with n_cols < cout on the split route: ldy != Cout
    "cols split": dict(d=(2, 8, 8, 40, 24, 5, 2), ncols=10, claims=dict(dgrad="split/nz4/cap_steps")),
    # the bias gradient's partials in the tail of the workspace, or -- with exactly the query -- the single kernel
    "tail partial": dict(d=(5, 30, 30, 10, 4, 3, 2), claims=dict(dbias="partial/nb3")),
    "tail narrow": dict(d=(5, 30, 30, 3, 4, 3, 2), h16=True, claims=dict(dbias="narrow/rpb1024/nb5")),
}

# linear: rcgan_linear_fwd / _bwd_data / _bwd_weight on (m, k, n).  sigma=False: a NULL sigma pointer.
LINEAR_CASES = {
    # two K-slices on 16 x 16 tiles, odd and even step counts; the dense filter gradient at m = 1024 (direct) and 1025 (slabs)
    "ks2 k264": dict(d=(1024, 264, 1024), claims=dict(fwd="gemm/ks2/odd", dgrad="split/nz3/cap_tiles", wgrad="direct/ks4/mod0", dbias="single")),
    "ks2 k288": dict(d=(1024, 288, 1024), h16=True, claims=dict(fwd="gemm/ks2/odd", wgrad="direct/ks4/mod0")),
    "ks2 k512": dict(d=(1024, 512, 1024), claims=dict(fwd="gemm/ks2/even")),
    "wgrad m1025": dict(d=(1025, 264, 1024), h16=True, claims=dict(wgrad="slabs/planned5/final5/cap_rows")),
    # the filter-gradient layout (N-major x N-major) under four K-slices with steps % 4 = 2 and 3 (0 and 1: above and below), and under
    # two K-slices (16 x 16 tiles) with an odd and an even step count
    "wgrad ks4 mod2": dict(d=(300, 264, 256), h16=True, claims=dict(wgrad="direct/ks4/mod2", fwd="gemm/ks4/mod1", dgrad="gemm/ks4/mod0")),
    "wgrad ks4 mod3": dict(d=(330, 264, 256), claims=dict(wgrad="direct/ks4/mod3")),
    "wgrad ks2 odd": dict(d=(264, 1024, 1024), claims=dict(wgrad="direct/ks2/odd")),
    "wgrad ks2 even": dict(d=(320, 1024, 1024), h16=True, claims=dict(wgrad="direct/ks2/even")),
    # n % 4 in {2, odd}, k % 8 != 0: lin_run4's three forms, lin_run8's clamped and zero-page tails
    "tails n990 k270": dict(d=(250, 270, 990), h16=True, claims=dict(fwd="gemm/ks4/mod1", dgrad="gemm/ks4/mod3", wgrad="direct/ks4/mod0")),
    "tails n989 k261": dict(d=(260, 261, 989), claims=dict(fwd="gemm/ks4/mod1", dgrad="gemm/ks4/mod3", wgrad="direct/ks4/mod1")),
    # dense data gradient, R = 2056: eight chunks, the last 40 long (two K-steps under four K-slices: groups 2 and 3 stage only zeros)
    "dgrad r2056": dict(d=(64, 1025, 2056), h16=True, claims=dict(dgrad="split/nz8/cap_8/last40/ks4/mod1"), claims16=dict(dgrad="gemm/ks4")),
    # linear_tiny on each side of 65536 / 65537 outputs and of 4096 / 4097 terms, in its three modes
    "tiny fwd out 65536": dict(d=(65536, 8, 1), h16=True, claims=dict(fwd="tiny", dgrad="gemm/ks1", wgrad="slabs/planned256/final256/cap_256", dbias="narrow/rpb1024/nb64")),
    "tiny fwd out 65537": dict(d=(65537, 8, 1), claims=dict(fwd="gemm/ks1")),
    "tiny red 4096": dict(d=(4, 4096, 17), h16=True, claims=dict(fwd="tiny", dgrad="tiny", wgrad="direct/ks1")),
    "tiny red 4097": dict(d=(4, 4097, 17), claims=dict(fwd="gemm/ks4/mod1")),
    "tiny dgrad red 4096": dict(d=(4, 17, 4096), h16=True, claims=dict(dgrad="tiny")),
    "tiny dgrad red 4097": dict(d=(4, 17, 4097), claims=dict(dgrad="split/nz8/cap_8")),
    "tiny dgrad out 65536": dict(d=(65536, 1, 8), claims=dict(dgrad="tiny", fwd="gemm/ks1")),
    "tiny dgrad out 65537": dict(d=(65537, 1, 8), claims=dict(dgrad="gemm/ks1")),
    "tiny wgrad out 65536": dict(d=(4, 65536, 1), claims=dict(wgrad="tiny")),
    "tiny wgrad out 65537": dict(d=(4, 65537, 1), h16=True, claims=dict(wgrad="direct/ks1")),
    # skinny forward at k = 511 / 512, n = 16 / 17, m = 1, with and without sigma
    "skinny k512 n16": dict(d=(1, 512, 16), h16=True, claims=dict(fwd="skinny")),
    "skinny k512 n16 no sigma": dict(d=(3, 515, 16), sigma=False, claims=dict(fwd="skinny")),
    "skinny k511": dict(d=(1, 511, 16), claims=dict(fwd="tiny")),
    "skinny n17": dict(d=(1, 512, 17), sigma=False, claims=dict(fwd="tiny")),
}
# column sums through the dense bias gradient (rows = m, c = n, k = 1), accumulate 0 / 1, fp32 and 16-bit
for _rows, _c, _claim in ([(2047, 8, "single"), (4096, 10, "single"), (2051, 64, "vec/rpb256/nb9/nrl32")]
                          + [(2048, c, "vec/rpb256/nb8/nrl%d" % (2048 // c)) for c in (8, 16, 32, 64, 128, 256)]
                          + [(4096, c, "narrow/rpb1024/nb4") for c in (1, 3, 7)]
                          + [(4097, c, "partial/nb3") for c in (10, 24, 138, 200)]
                          + [(262145, 8, "vec/rpb512/nb513/nrl256")]):
    LINEAR_CASES["colsum %d x %d" % (_rows, _c)] = dict(d=(_rows, 1, _c), h16=True, claims=dict(dbias=_claim))

# the two shapes outside the tables: the label-column filter gradient (n, h, w, cin, c1, c2, k, stride) and the captured convolution
LABEL_SHAPE = (33, 14, 14, 8, 64, 10, 5, 2)
REPLAY_SHAPE = (5, 8, 8, 993, 16, 1, 1)

# what the tables must reach between them: (call, branch) with the branch a prefix or "prefix*suffix".  Every K-slice row for the three
# layout pairs: K x N (fwd), K x K (dgrad), N x N (wgrad, whether it writes slabs or straight into the gradient)
BRANCHES = ([("fwd", "gemm/ks1"), ("fwd", "gemm/ks2/odd"), ("fwd", "gemm/ks2/even"), ("dgrad", "gemm/ks1"), ("dgrad", "gemm/ks2/even"), ("dgrad", "gemm/ks2/odd"),
             ("wgrad", "direct/ks4"), ("wgrad", "direct/ks1"), ("wgrad", "*/ks1"), ("wgrad", "slabs*/ks2/odd"), ("wgrad", "slabs*/ks2/even"),
             ("wgrad", "direct/ks2/odd"), ("wgrad", "direct/ks2/even"), ("vec", "x4dy4"), ("vec", "x2dy2"), ("vec", "x1dy1"), ("chunks", "5")]
            + [(op, "gemm/ks4/mod%d" % r) for op in ("fwd", "dgrad") for r in range(4)] + [("wgrad", "*/ks4/mod%d" % r) for r in range(4)]
            + [("fwd", "split/nz4/cap_steps"), ("fwd", "split/nz2/cap_tiles"), ("fwd", "split/nz8/cap_8"), ("dgrad", "split/nz8/cap_8/last40/ks4"),
               ("dgrad", "split/nz4/cap_steps"), ("fwd", "two_step/split"), ("dgrad", "two_step/tiny"), ("dgrad", "narrow/vec4"), ("dgrad", "narrow/vec2"),
               ("dgrad", "narrow/vec1"), ("dgrad", "s2gemm/ks1/cls4/zero0"), ("dgrad", "s2gemm/ks1/cls4/zero3"), ("dgrad", "s2gemm/ks1/cls2"),
               ("dgrad", "s2gemm/ks4"), ("dgrad", "narrow/vec4/cls4/zero3"),
               ("wgrad", "slabs/planned1/final1"), ("wgrad", "slabs/planned2/"), ("wgrad", "slabs/planned3/"), ("wgrad", "slabs/planned17/"),
               ("wgrad", "slabs/planned64/final64/cap_rows"), ("wgrad", "slabs/planned16/final16/cap_tiles"), ("wgrad", "slabs/planned6/final6/cap_fit"),
               ("wgrad", "slabs/planned5/final5/cap_rows"), ("wgrad", "slabs/planned16/final16/cap_rows/last10/"), ("wgrad", "slabs/planned256/final241"),
               ("wgrad", "slabs/planned256/final256/cap_256"), ("wgrad", "tiny"),
               ("dbias", "single"), ("dbias", "vec/rpb256"), ("dbias", "vec/rpb512"), ("dbias", "narrow/rpb1024"), ("dbias", "narrow/rpb2048"), ("dbias", "narrow/rpb4096"),
               ("dbias", "partial/"), ("fwd", "tiny"), ("fwd", "skinny"), ("dgrad", "tiny")]
            + [("dbias", "vec/rpb256/nb8/nrl%d" % r) for r in (256, 128, 64, 32, 16, 8)])


def matches(branch, claim):
    """claim: a prefix of the branch, or "prefix*suffix"."""
    head, _, tail = claim.partition("*")
    return branch.startswith(head) and branch.endswith(tail)


def _claims_of(case, dt):
    """f32: the table's claims; h16: those that do not name an fp32-only route (split reduction, two-step), plus the case's claims16."""
    if dt == "f32" or case.get("only16"):
        return case["claims"]
    out = {k: v for k, v in case["claims"].items() if not v.startswith(("split", "two_step"))}
    out.update(case.get("claims16", {}))
    return out


def plan_claims():
    """(case id, line for `gather_plan_sweep cases`, {call: claimed prefix}) for every case; f32 lines, and h16 lines for the 16-bit cases."""
    out = []
    for kind, table in (("conv", CONV_CASES), ("deconv", DECONV_CASES), ("linear", LINEAR_CASES)):
        for name, c in table.items():
            for dt in (["f32"] if not c.get("only16") else []) + (["h16"] if c.get("h16") else []):
                tail = {"conv": (c.get("mask", 0), c.get("off", 0)), "deconv": (c.get("ncols", 0), 1), "linear": ()}[kind]
                out.append(("%s %s %s" % (kind, name, dt), " ".join([kind, dt] + [str(v) for v in c["d"] + tail]), _claims_of(c, dt)))
                if kind == "deconv":
                    # the pass with exactly rcgan_conv_workspace_bytes: no tail, the single kernel; `tail`: _tail_bytes pinned to the header's
                    n, h, w, cin = c["d"][:4]
                    out.append(("deconv %s %s, no tail" % (name, dt), " ".join(["deconv", dt] + [str(v) for v in c["d"] + (c.get("ncols", 0), 0)]),
                                dict(dbias="single*single", tail="%d*%d" % ((_tail_bytes(n * h * w, cin),) * 2))))
    for dt in ("f32", "h16"):
        out.append(("label columns %s" % dt, " ".join(["concat", dt] + [str(v) for v in LABEL_SHAPE]),
                    dict(wgrad="slabs/planned7/final7/cap_rows", dbias="vec/rpb256/nb26/nrl256", chunks="5*5")))
    out.append(("graph replay f32", " ".join(["conv", "f32"] + [str(v) for v in REPLAY_SHAPE + (0, 0)]), dict(fwd="split/nz4/cap_steps", wgrad="slabs/planned2/final2/")))
    return out


# ---------------------------------------------------------------------------------------------------- contexts
MODES = ["f32", "f32high", "bf16", "f16"]


@pytest.fixture(scope="module")
def _contexts():
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx("f32" if mode.startswith("f32") else mode, arena=1 << 20)      # (its own arena is replaced by the guarded one)
            if mode == "f32high":
                ctx.set_f32_matmul_precision("high")
            cm = guarded(ctx, arena_bytes=768 << 20, ws_bytes=64 << 20)
            ctx.guard = cm.__enter__()
            made[mode] = (ctx, cm)
        return made[mode][0], mode

    yield get
    for ctx, cm in made.values():
        cm.__exit__(None, None, None)
        ctx.close()


def _pairs(table):
    """(mode, case name) for every context a row of the table runs in."""
    out = []
    for name in sorted(table):
        c = table[name]
        out += [(m, name) for m in MODES if (m.startswith("f32") and not c.get("only16")) or (not m.startswith("f32") and c.get("h16"))]
    return out


def _ids(pairs):
    return ["%s-%s" % p for p in pairs]


# ---------------------------------------------------------------------------------------------------- helpers
def _p(t):
    return C.c_void_p(t.ptr) if t is not None else None


def _ints(rs, shape, lim):
    return rs.randint(-lim, lim + 1, size=shape).astype(np.float64)


def _up(ctx, arr, dtype=None, off=0):
    """Upload; off > 0: the tensor starts that many elements into its allocation (a base pointer that is not 16-byte aligned)."""
    from rcgan_amd.runtime import DT
    arr = np.asarray(arr)
    if not off:
        return ctx.upload(arr, dtype)
    whole = ctx.empty((arr.size + 8,), dtype)
    t = DT(whole.ptr + off * whole.itemsize, arr.shape, whole.dtype, whole.base)
    return ctx.upload(arr, dtype, out=t)


class Pass:
    """One pass of a case: launches into 0xFF-filled (or integer / gaussian pre-filled) outputs, then one sync, the bands, every output."""

    def __init__(self, ctx, mode, exact, what):
        self.ctx, self.mode, self.exact, self.what, self.todo = ctx, mode, exact, what, []
        self.m16 = mode if mode in ("bf16", "f16") else "f32"

    def out(self, rs, shape, acc, dtype=None):
        """(tensor, what it held before as float64): a fresh output, or an accumulate target."""
        if not acc:
            return self.ctx.empty(shape, dtype), 0.0
        prev = _ints(rs, shape, 3) if self.exact else rs.randn(*shape)
        prev = np.asarray(half_round(self.m16 if dtype is None else "f32", prev), np.float64)
        return self.ctx.upload(prev, dtype), prev

    def expect(self, name, t, ref, bound, kind):
        """kind "act": stored in the activation dtype, tolerance TOL[mode]; "grad": fp32, 2e-4.  bound: the reference of |inputs|."""
        if self.exact:
            assert np.abs(bound).max() < 2 ** 24, "%s %s: partial sums reach %g, not exact in fp32" % (self.what, name, np.abs(bound).max())
        self.todo.append((name, t, np.asarray(ref, np.float64), kind))

    def done(self):
        ctx, g = self.ctx, self.ctx.guard
        ctx.sync()
        g.check()
        for name, t, ref, kind in self.todo:
            what = "%s %s (%s, %s)" % (self.what, name, self.mode, "exact" if self.exact else "gaussian")
            assert g.unwritten(t) == 0, "%s: %d elements never written" % (what, g.unwritten(t))
            got = np.asarray(ctx.download(t), np.float64)
            if self.exact:
                want = np.asarray(half_round(self.m16, ref), np.float64) if kind == "act" else ref
                bad = got != want
                assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r, want %r" % (
                    what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])
            else:
                tol = TOL[self.m16] if kind == "act" else 2e-4
                err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12)
                print("%s: max err %.3e of max|ref| (tolerance %.1e)" % (what, err, tol))
                assert_close(got, ref, tol, what)
        self.todo = []


def _inputs(rs, mode, exact, shape, lim=3, scale=1.0):
    if exact:
        return _ints(rs, shape, lim)
    m16 = mode if mode in ("bf16", "f16") else "f32"
    return np.asarray(half_round(m16, rs.randn(*shape) * scale), np.float64)


def _workspaces(ctx, sizes):
    """The production-like workspace, then a region of exactly each of `sizes` bytes."""
    import contextlib
    yield "default", contextlib.nullcontext()
    for s in sizes:
        yield "%d bytes" % s, ctx.guard.workspace(s)


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


# ---------------------------------------------------------------------------------------------------- convolutions
def _run_conv(ctx, mode, name, case, exact, acc):
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    n, h, w, cin, cout, k, s = case["d"]
    mask, off = case.get("mask", 0), case.get("off", 0)
    lib, dt = ctx.lib, ctx.act_dtype
    flags = L.CONV_FORCE_DIRECT | (L.CONV_IN_RELU if mask else 0)
    desc = L.ConvDesc(n, h, w, cin, cout, k, k, s, dt, flags)
    adesc = L.ConvDesc(n, h, w, cin, cout, k, k, s, dt, flags | (L.CONV_ACCUMULATE if acc else 0))
    oh, ow = nn.same_pad(h, k, s)[0], nn.same_pad(w, k, s)[0]
    if not exact and max(k * k * cin, k * k * cout, n * oh * ow) > 8192:      # a long reduction: the exact pass alone
        return
    rs = np.random.RandomState(_seed(name))
    sigma = np.float32(0.5 if exact else 1.7)
    x = _inputs(rs, mode, exact, (n, h, w, cin))
    wgt = _ints(rs, (k, k, cin, cout), 2) if exact else (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32).astype(np.float64)
    b = _inputs(rs, "f32", exact, (cout,)).astype(np.float32).astype(np.float64)
    w_eff = wgt / np.float64(sigma)
    xin = np.maximum(x, 0) if mask else x
    yref = nn.conv2d_fwd(xin, w_eff, s)
    dy = _inputs(rs, mode, exact, yref.shape)
    dxref = nn.conv2d_bwd_input(dy, w_eff, x.shape, s) * ((x > 0) if mask else 1.0)
    dwref = nn.conv2d_bwd_filter(xin, dy, wgt.shape, s)
    ab = (lambda f, *a: f(*a)) if exact else (lambda f, *a: 0.0)      # the references of |inputs|: bounds of every partial sum
    ybound = ab(lambda: nn.conv2d_fwd(np.abs(xin), np.abs(w_eff), s) + np.abs(b) + 3)
    dxbound = ab(lambda: nn.conv2d_bwd_input(np.abs(dy), np.abs(w_eff), x.shape, s) + 3)
    dwbound = ab(lambda: nn.conv2d_bwd_filter(np.abs(xin), np.abs(dy), wgt.shape, s) + 3)
    ws_need = lib.rcgan_conv_workspace_bytes(C.byref(desc))
    for ws_name, ws_cm in _workspaces(ctx, [ws_need]):
        with ws_cm:
            ctx.guard.clear()
            P = Pass(ctx, mode, exact, "conv [%s] acc %d, workspace %s," % (name, acc, ws_name))
            xd, dyd = _up(ctx, x, off=off), _up(ctx, dy, off=off)
            wp = ctx.guard.persistent(wgt.shape, L.F32)
            ctx.upload(wgt, L.F32, out=wp)
            bd = ctx.upload(b, L.F32)
            sg = ctx.upload(np.array([sigma], np.float32), L.F32)
            prep = O.Weight(ctx, wp, sg).prepared(desc)
            y, yprev = P.out(rs, yref.shape, acc)
            ctx.check(lib.rcgan_conv2d_fwd(ctx.h, C.byref(adesc), _p(xd), _p(prep), _p(bd), _p(y)))
            P.expect("forward", y, yref + b + yprev, ybound, "act")
            dx, dxprev = P.out(rs, x.shape, acc)
            ctx.check(lib.rcgan_conv2d_bwd_data(ctx.h, C.byref(adesc), _p(dyd), _p(prep), _p(xd) if mask else None, _p(dx), C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            P.expect("data gradient", dx, dxref + dxprev, dxbound, "act")
            dw, dwprev = P.out(rs, wgt.shape, acc, L.F32)
            db, dbprev = P.out(rs, (cout,), acc, L.F32)
            ctx.check(lib.rcgan_conv2d_bwd_weight(ctx.h, C.byref(desc), _p(xd), _p(dyd), _p(dw), _p(db), acc, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            P.expect("filter gradient", dw, dwref + dwprev, dwbound, "grad")
            P.expect("bias gradient", db, dy.sum(axis=(0, 1, 2)) + dbprev, np.abs(dy).sum(axis=(0, 1, 2)) + 3, "grad")
            P.done()


@pytest.mark.parametrize("mode,name", _pairs(CONV_CASES), ids=_ids(_pairs(CONV_CASES)))
def test_conv(_contexts, mode, name):
    ctx, mode = _contexts(mode)
    case = CONV_CASES[name]
    _run_conv(ctx, mode, name, case, True, 0)
    _run_conv(ctx, mode, name, case, True, 1)
    _run_conv(ctx, mode, name, case, False, 0)


def test_grid_limit_refusal(_contexts):
    """One row tile past the grid limit (256 * 256 * 64 rows): RCGAN_EUNSUPPORTED_SHAPE before any launch, nothing written."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx, mode = _contexts("f32")
    n, h, w = 256, 256, 64
    desc = L.ConvDesc(n, h, w, 1, 1, 1, 1, 1, ctx.act_dtype, L.CONV_FORCE_DIRECT)
    ctx.guard.clear()
    x = ctx.upload(np.ones((n, h, w, 1), np.float32))
    wp = ctx.guard.persistent((1, 1, 1, 1), L.F32, fill=1.0)
    prep = O.Weight(ctx, wp, None).prepared(desc)
    y, dx = ctx.empty((n, h, w, 1)), ctx.empty((n, h, w, 1))
    assert ctx.lib.rcgan_conv2d_fwd(ctx.h, C.byref(desc), _p(x), _p(prep), None, _p(y)) == L.EUNSUPPORTED_SHAPE
    assert ctx.lib.rcgan_conv2d_bwd_data(ctx.h, C.byref(desc), _p(x), _p(prep), None, _p(dx), C.c_void_p(ctx.ws_ptr), ctx.ws_bytes) == L.EUNSUPPORTED_SHAPE
    ctx.sync()
    ctx.guard.check()
    assert ctx.guard.unwritten(y) == y.size and ctx.guard.unwritten(dx) == dx.size


# ---------------------------------------------------------------------------------------------------- transposed convolutions
def _tail_bytes(rows, c):
    """The column-sum tail rcgan_deconv2d_bwd_weight looks for behind rcgan_conv_workspace_bytes (csrc/gather_plan.h: colsum_tail_bytes)."""
    return (((rows + 2047) // 2048 + 1024) * c * 4 + 255) // 256 * 256


def _run_deconv(ctx, mode, name, case, exact, acc):
    from rcgan_amd import _lib as L
    n, h, w, cin, cout, k, s = case["d"]
    ncols = case.get("ncols", 0)
    lib, dt = ctx.lib, ctx.act_dtype
    desc = L.ConvDesc(n, h, w, cin, cout, k, k, s, dt, 0)
    adesc = L.ConvDesc(n, h, w, cin, cout, k, k, s, dt, L.CONV_ACCUMULATE if acc else 0)
    oh, ow = nn.same_pad(h, k, s)[0], nn.same_pad(w, k, s)[0]
    if not exact and max(k * k * cin, k * k * cout, n * oh * ow, n * h * w) > 8192:      # a long reduction: the exact pass alone
        return
    rs = np.random.RandomState(_seed(name))
    x = _inputs(rs, mode, exact, (n, oh, ow, cout))                      # the transposed convolution's input
    wgt = _ints(rs, (k, k, cin, cout), 2) if exact else (rs.randn(k, k, cin, cout) * 0.05).astype(np.float32).astype(np.float64)
    b = _inputs(rs, "f32", exact, (cin,)).astype(np.float32).astype(np.float64)
    dy = _inputs(rs, mode, exact, (n, h, w, cin))                        # gradient of its output
    yref = nn.conv2d_bwd_input(x, wgt, dy.shape, s) + b
    nc = ncols or cout
    dxref = nn.conv2d_fwd(dy, wgt, s)[..., :nc]
    dwref = nn.conv2d_bwd_filter(dy, x, wgt.shape, s)
    ab = (lambda f: f()) if exact else (lambda f: 0.0)
    ybound = ab(lambda: nn.conv2d_bwd_input(np.abs(x), np.abs(wgt), dy.shape, s) + np.abs(b))
    dxbound = ab(lambda: nn.conv2d_fwd(np.abs(dy), np.abs(wgt), s) + 3)
    dwbound = ab(lambda: nn.conv2d_bwd_filter(np.abs(dy), np.abs(x), wgt.shape, s) + 3)
    q = lib.rcgan_conv_workspace_bytes(C.byref(desc))
    for ws_name, ws_cm in _workspaces(ctx, [q, q + _tail_bytes(n * h * w, cin)]):
        with ws_cm:
            ctx.guard.clear()
            P = Pass(ctx, mode, exact, "deconv [%s] acc %d, workspace %s," % (name, acc, ws_name))
            xd, dyd, wd, bd = ctx.upload(x), ctx.upload(dy), ctx.upload(wgt, L.F32), ctx.upload(b, L.F32)
            if not acc:                                                  # (the forward never accumulates)
                y = ctx.empty(dy.shape)
                ctx.check(lib.rcgan_deconv2d_fwd(ctx.h, C.byref(desc), _p(xd), _p(wd), _p(bd), _p(y)))
                P.expect("forward", y, yref, ybound, "act")
            dx, dxprev = P.out(rs, dxref.shape, acc)
            ctx.check(lib.rcgan_deconv2d_bwd_data_cols(ctx.h, C.byref(adesc), _p(dyd), _p(wd), _p(dx), ncols))
            P.expect("data gradient", dx, dxref + dxprev, dxbound, "act")
            dw, dwprev = P.out(rs, wgt.shape, acc, L.F32)
            db, dbprev = P.out(rs, (cin,), acc, L.F32)
            ctx.check(lib.rcgan_deconv2d_bwd_weight(ctx.h, C.byref(desc), _p(xd), _p(dyd), _p(dw), _p(db), acc, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            P.expect("filter gradient", dw, dwref + dwprev, dwbound, "grad")
            P.expect("bias gradient", db, dy.sum(axis=(0, 1, 2)) + dbprev, np.abs(dy).sum(axis=(0, 1, 2)) + 3, "grad")
            P.done()


@pytest.mark.parametrize("mode,name", _pairs(DECONV_CASES), ids=_ids(_pairs(DECONV_CASES)))
def test_deconv(_contexts, mode, name):
    ctx, mode = _contexts(mode)
    case = DECONV_CASES[name]
    _run_deconv(ctx, mode, name, case, True, 0)
    _run_deconv(ctx, mode, name, case, True, 1)
    _run_deconv(ctx, mode, name, case, False, 0)


def _run_label_columns(ctx, mode, exact, acc):
    """rcgan_deconv2d_bwd_weight_concat at n = 33 (five sample chunks of the label-column product): the transposed convolution's input is
    [t ; yb broadcast over the pixels], c1 = 64 real and c2 = 10 label channels; 7 slabs over the real columns, the bias gradient's
    partials (8-wide route) in the workspace's tail."""
    from rcgan_amd import _lib as L
    n, h, w, cin, c1, c2, k, s = LABEL_SHAPE
    lib, dt = ctx.lib, ctx.act_dtype
    desc = L.ConvDesc(n, h, w, cin, c1 + c2, k, k, s, dt, 0)
    oh, ow = nn.same_pad(h, k, s)[0], nn.same_pad(w, k, s)[0]
    rs = np.random.RandomState(33 + acc)
    t = _inputs(rs, mode, exact, (n, oh, ow, c1))
    yb = _ints(rs, (n, c2), 3) if exact else rs.rand(n, c2).astype(np.float32).astype(np.float64)
    dy = _inputs(rs, mode, exact, (n, h, w, cin))
    xfull = np.concatenate([t, np.broadcast_to(yb[:, None, None, :], (n, oh, ow, c2))], axis=3)
    m16 = mode if mode in ("bf16", "f16") else "f32"
    xdev = np.concatenate([t, half_round(m16, np.broadcast_to(yb[:, None, None, :], (n, oh, ow, c2)))], axis=3)   # (the kernel reads yb, not these)
    wshape = (k, k, cin, c1 + c2)
    dwref = nn.conv2d_bwd_filter(dy, xfull, wshape, s)
    dwbound = nn.conv2d_bwd_filter(np.abs(dy), np.abs(xfull), wshape, s) + 3 if exact else 0.0
    for ws_name, ws_cm in _workspaces(ctx, [lib.rcgan_deconv2d_bwd_weight_concat_bytes(C.byref(desc), c1)]):
        with ws_cm:
            ctx.guard.clear()
            P = Pass(ctx, mode, exact, "label columns acc %d, workspace %s," % (acc, ws_name))
            xd, dyd, ybd = ctx.upload(xdev), ctx.upload(dy), ctx.upload(yb, L.F32)
            dw, dwprev = P.out(rs, wshape, acc, L.F32)
            db, dbprev = P.out(rs, (cin,), acc, L.F32)
            ctx.check(lib.rcgan_deconv2d_bwd_weight_concat(ctx.h, C.byref(desc), _p(xd), _p(dyd), c1, _p(ybd), _p(dw), _p(db), acc,
                                                           C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            P.expect("filter gradient", dw, dwref + dwprev, dwbound, "grad")
            P.expect("bias gradient", db, dy.sum(axis=(0, 1, 2)) + dbprev, np.abs(dy).sum(axis=(0, 1, 2)) + 3, "grad")
            P.done()


@pytest.mark.parametrize("mode", MODES)
def test_deconv_label_columns(_contexts, mode):
    ctx, mode = _contexts(mode)
    _run_label_columns(ctx, mode, True, 0)
    _run_label_columns(ctx, mode, True, 1)
    _run_label_columns(ctx, mode, False, 0)


# ---------------------------------------------------------------------------------------------------- dense layers
def _run_linear(ctx, mode, name, case, exact, acc):
    from rcgan_amd import _lib as L
    m, k, n = case["d"]
    lib, dt = ctx.lib, ctx.act_dtype
    if not exact and max(m, k, n) > 8192:      # a long reduction: the exact pass alone
        return
    rs = np.random.RandomState(_seed(name))
    has_sigma = case.get("sigma", True)
    sigma = np.float32((0.5 if exact else 1.7) if has_sigma else 1.0)
    x = _inputs(rs, mode, exact, (m, k))
    wgt = _ints(rs, (k, n), 2) if exact else (rs.randn(k, n) / np.sqrt(k)).astype(np.float32).astype(np.float64)
    b = _inputs(rs, "f32", exact, (n,)).astype(np.float32).astype(np.float64)
    dy = _inputs(rs, mode, exact, (m, n))
    w_eff = wgt / np.float64(sigma)
    ab = (lambda f: f()) if exact else (lambda f: 0.0)
    q = lib.rcgan_linear_workspace_bytes(m, k, n)
    for ws_name, ws_cm in _workspaces(ctx, [q]):
        with ws_cm:
            ctx.guard.clear()
            P = Pass(ctx, mode, exact, "linear [%s] acc %d, workspace %s," % (name, acc, ws_name))
            xd, dyd, wd, bd = ctx.upload(x), ctx.upload(dy), ctx.upload(wgt, L.F32), ctx.upload(b, L.F32)
            sg = ctx.upload(np.array([sigma], np.float32), L.F32) if has_sigma else None
            if not acc:                                                  # (the forward never accumulates)
                y = ctx.empty((m, n))
                ctx.check(lib.rcgan_linear_fwd(ctx.h, m, k, n, dt, _p(xd), _p(wd), _p(sg), _p(bd), _p(y)))
                P.expect("forward", y, x @ w_eff + b, ab(lambda: np.abs(x) @ np.abs(w_eff) + np.abs(b)), "act")
            dx, dxprev = P.out(rs, (m, k), acc)
            ctx.check(lib.rcgan_linear_bwd_data(ctx.h, m, k, n, dt, _p(dyd), _p(wd), _p(sg), _p(dx), acc))
            P.expect("data gradient", dx, dy @ w_eff.T + dxprev, ab(lambda: np.abs(dy) @ np.abs(w_eff).T + 3), "act")
            dw, dwprev = P.out(rs, (k, n), acc, L.F32)
            db, dbprev = P.out(rs, (n,), acc, L.F32)
            ctx.check(lib.rcgan_linear_bwd_weight(ctx.h, m, k, n, dt, _p(xd), _p(dyd), _p(dw), _p(db), acc, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
            P.expect("filter gradient", dw, x.T @ dy + dwprev, ab(lambda: np.abs(x).T @ np.abs(dy) + 3), "grad")
            P.expect("bias gradient", db, dy.sum(0) + dbprev, np.abs(dy).sum(0) + 3, "grad")
            P.done()


@pytest.mark.parametrize("mode,name", _pairs(LINEAR_CASES), ids=_ids(_pairs(LINEAR_CASES)))
def test_linear(_contexts, mode, name):
    ctx, mode = _contexts(mode)
    case = LINEAR_CASES[name]
    _run_linear(ctx, mode, name, case, True, 0)
    _run_linear(ctx, mode, name, case, True, 1)
    _run_linear(ctx, mode, name, case, False, 0)


# ---------------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("mode", ["f32", "f32high"])
def test_graph_replay(_contexts, mode):
    """A split-reduction forward and a sliced filter gradient (nz > 1), captured after an eager run of the same shapes has sized the
    grow-only scratch; each graph replayed twice gives the eager bytes."""
    from rcgan_amd import _lib as L
    from rcgan_amd import ops as O
    ctx, mode = _contexts(mode)
    n, h, w, cin, cout = REPLAY_SHAPE[:5]          # forward: 5 tiles, 4 chunks; filter gradient: M = 320, 2 slabs
    desc = L.ConvDesc(n, h, w, cin, cout, 1, 1, 1, ctx.act_dtype, L.CONV_FORCE_DIRECT)
    rs = np.random.RandomState(5)
    ctx.guard.clear()
    x, dy = ctx.upload(rs.randn(n, h, w, cin)), ctx.upload(rs.randn(n, h, w, cout))
    wp = ctx.guard.persistent((1, 1, cin, cout), L.F32)
    ctx.upload(rs.randn(1, 1, cin, cout) / 30, L.F32, out=wp)
    b = ctx.upload(rs.randn(cout), L.F32)
    prep = O.Weight(ctx, wp, None).prepared(desc)
    outs = [(ctx.empty((n, h, w, cout)), ctx.empty((1, 1, cin, cout), L.F32), ctx.empty((cout,), L.F32)) for _ in range(2)]

    def launch(y, dw, db):
        ctx.check(ctx.lib.rcgan_conv2d_fwd(ctx.h, C.byref(desc), _p(x), _p(prep), _p(b), _p(y)))
        ctx.check(ctx.lib.rcgan_conv2d_bwd_weight(ctx.h, C.byref(desc), _p(x), _p(dy), _p(dw), _p(db), 0, C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))

    launch(*outs[0])                       # eager: sizes the scratch
    ctx.sync()
    eager = [ctx.download(t).copy() for t in outs[0]]
    ctx.graph_begin()
    try:
        launch(*outs[1])
    except Exception:
        ctx.graph_abort()
        raise
    gid = ctx.graph_end()
    for _ in range(2):
        ctx.graph_launch(gid)
        ctx.sync()
        ctx.guard.check()
        for t, e in zip(outs[1], eager):
            assert ctx.guard.unwritten(t) == 0
            assert np.array_equal(ctx.download(t).view(np.uint32), e.view(np.uint32)), "replay differs from the eager run"
