"""The batch-norm planner (csrc/bn_plan.h) swept without a GPU: tests/tools/bn_plan_sweep.cpp, built with the host C++ compiler and
-fsanitize=address,undefined, run as a child process -- nothing is loaded into this interpreter.  One run has RCGAN_BN_TREE_MIN at the
value tests/conftest.py gives the GPU tests (the tree route on offer), one has it unset (production).

Checked: the invariants the program asserts over its grid (groups cover the rows and never straddle a sample, workspace regions are
disjoint and within `need`, `need` within the documented query for n <= 8192, grid and LDS and counter-line limits, the fused apply's
stride, BN_VEC only where its tables fit, index types); that every case of tests/test_gpu_bn_edges.py reaches the route and branch its
table names, and the tables together every branch listed there; the figures that file and include/rcgan_hip.h quote from the sweep."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import test_gpu_bn_edges as E
from tests import test_gpu_many_classes_ops as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "tools", "bn_plan_sweep.cpp")
TREE_MIN = os.environ["RCGAN_BN_TREE_MIN"]         # tests/conftest.py


@pytest.fixture(scope="module")
def sweep_program(tmp_path_factory):
    cxx = next((p for p in (shutil.which(n) for n in (os.environ.get("CXX") or "c++", "g++", "clang++")) if p), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("bn_plan") / "bn_plan_sweep")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # the sanitizer runtimes linked statically where the compiler offers it, dynamically otherwise
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if subprocess.run([cxx] + flags + static + ["-o", exe, SOURCE], capture_output=True).returncode == 0:
            return exe
    subprocess.run([cxx] + flags + ["-o", exe, SOURCE], check=True)      # (shows the compiler's message)


def _run(exe, mode, tree, stdin=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RCGAN_BN_")}
    if tree:
        env["RCGAN_BN_TREE_MIN"] = TREE_MIN
    return subprocess.run([exe, mode], input=stdin, env=env, capture_output=True, text=True, timeout=600)


def _fields(line):
    return dict(f.split("=", 1) for f in line.split()[1:] if "=" in f)


@pytest.fixture(scope="module")
def sweeps(sweep_program):
    return {tree: _run(sweep_program, "sweep", tree) for tree in (True, False)}


@pytest.mark.parametrize("tree", [True, False])
def test_planner_invariants_hold_over_the_grid(sweeps, tree):
    r = sweeps[tree]
    assert r.returncode == 0 and "violations 0" in r.stdout and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) > 2000000, "the sweep planned %s calls" % last[1]
    assert (last[-1] == TREE_MIN) == tree, last
    routes = {l.split()[1] for l in r.stdout.splitlines() if l.startswith("swept ")}
    want = {"STATS/COLUMN", "STATS/VEC", "STATS/SCALAR", "APPLY/COLUMN", "APPLY/VEC", "APPLY/SCALAR", "BWD/COLUMN", "BWD/VEC", "BWD/SCALAR", "BWD/WIDE",
            "STATS_SEG/COLUMN", "STATS_SEG/per_segment", "APPLY_SEG/COLUMN", "APPLY_SEG/per_segment"}
    if tree:
        want |= {"STATS/TREE", "BWD/TREE", "STATS_SEG/TREE"}
    assert want <= routes and (tree or not any(k.endswith("/TREE") for k in routes)), routes


def test_figures_quoted_from_the_sweep(sweeps):
    """first_exceed: the n of test_gpu_bn_edges.FIRST_EXCEED and of the rcgan_bn_bwd comment in include/rcgan_hip.h; halving: the rows of
    test_gpu_bn_edges.HALVINGS; the fused apply never has more than 256 chunks per row (the branch bn_apply_grid used to have for it)."""
    out = sweeps[False].stdout
    first = {}
    for l in out.splitlines():
        if l.startswith("first_exceed "):
            f = _fields(l)
            first[(f["route"], int(f["rps"]), int(f["c"]), int(f["n_labels"]))] = int(f["n"])
    for key, n in E.FIRST_EXCEED.items():
        assert first[key] == n, (key, first[key])
    # what the header of rcgan_bn_bwd says, as formulas in c and n_labels: never at or below 8192; per route with a workspace to spare ...
    from fractions import Fraction as F
    after = lambda bound: int(bound // 1) + 1                        # the first integer past a bound
    assert min(v for v in first.values() if v) > 8192
    for (route, rps, c, K), n in first.items():
        want = {"COLUMN": after(8209 + F(32, c)), "SCALAR": after(8209 + F(32, c)), "VEC": after(8208 - F(K, 2) + F(32, c)),
                "WIDE": after(8208 + max(K - 16, 0) + F(32, c)), "TREE": 0}[route]
        if n:                                                          # (c = 16 is never BN_SCALAR with a workspace to spare)
            assert n == want, (route, rps, c, K, n, want)
    assert first[("SCALAR", 1, 100, 10)] == first[("SCALAR", 1, 33, 10)] == 8210 and first[("SCALAR", 1, 31, 2)] == 8211
    # ... and with exactly the query's bytes: where the c % 8 == 0 route loses its tables, where the call is refused, by which route
    seen = 0
    for l in out.splitlines():
        if l.startswith("first_refused "):
            f = _fields(l)
            c, K = int(f["c"]), int(f["n_labels"])
            fused = c >= 64 and c & (c - 1) == 0
            tables = K <= 16 and c % 8 == 0 and not fused
            assert int(f["tables_lost"]) == (after(8208 - F(K, 2) + F(32, c)) if tables else 0), l
            assert int(f["n"]) == (8210 + 32 // c if K <= 16 else 8209 + (K - 16) + 32 // c), l
            assert f["route"] == ("WIDE" if K > 16 else "COLUMN" if fused else "SCALAR"), l
            seen += 1
    assert seen >= 200
    with open(os.path.join(ROOT, "include", "rcgan_hip.h")) as fh:
        header = " ".join(fh.read().split())
    for text in ("which covers every * n <= 8192", "from the first n > 8208 - n_labels/2 + 32/c (16 labels, c >= 40: 8201)",
                 "from n = 8210 + floor(32/c) for n_labels <= 16 (c >= 33: 8210, c = 17 .. 32: * 8211)",
                 "from n = 8209 + (n_labels - 16) + floor(32/c) for n_labels > 16",
                 "(n + 1)*2*c on the scalar and the power-of-two-c routes, (n + 2)*2*c on the * per-sample route"):
        assert text in header, text
    halving = {}
    for l in out.splitlines():
        if l.startswith("halving "):
            f = _fields(l)
            halving.setdefault(int(f["c"]), (int(f["rows"]), int(f["rpg_below"]), int(f["rpg_at"])))      # the first step of each c
    assert halving == E.HALVINGS
    assert "max_fused_chunks_per_row 256" in out
    # with the tree on offer a labelled backward never needs more than the query because of the tree
    tree_first = [l for l in sweeps[True].stdout.splitlines() if l.startswith("first_exceed route=TREE")]
    assert tree_first and all(" n=0 " in l for l in tree_first), tree_first


def test_edge_cases_reach_the_branches_they_name(sweep_program):
    claims = E.plan_claims()
    r = _run(sweep_program, "cases", True, "\n".join(line for _, line, _ in claims) + "\n")
    assert r.returncode == 0 and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("case ")]
    assert len(lines) == len(claims)
    reached = set()
    for (name, line, expect), got in zip(claims, lines):
        f = _fields(got)
        for k, v in expect.items():
            assert f[k] == v, "%s (%s): %s is %s, the table says %s\n%s" % (name, line, k, f[k], v, got)
        n, rps, c, K = (int(t) for t in line.split()[2:6])
        assert int(f["query"]) == int(line.split()[1]) * E.query_bytes(n * rps, c, K), "the two restatements of the query differ: " + line
        assert int(f["need"]) <= int(f["query"]) or name.startswith("contract"), got
        if name.startswith("contract"):
            assert int(f["need"]) > int(f["query"]) or f["route"] == "SCALAR", got
        reached.add((f["route"], f["branch"]))
        reached.add(("apply", f["apply"], f["strides"]))
        reached.add(("nsub", f["nsub"]))
    missing = [b for b in E.BRANCHES if b not in reached]
    assert not missing, missing


def test_production_has_no_tree(sweep_program):
    """The same table without the switch: what the tree took goes to the column kernels."""
    r = _run(sweep_program, "cases", False, "BWD 1 %d %d %d 16 1 1 query\nSTATS 1 1 %d %d 1 0 1 query\n" % (E.TREE_SHAPE + E.STATS_TREE))
    assert r.returncode == 0 and r.stdout.count("route=COLUMN") == 2, r.stdout + r.stderr


def test_reference_restatement():
    """bn_ref / bn_ref_bwd of the GPU file (per-sample sums first) against test_gpu_many_classes_ops._bn_ref on a small case."""
    rs = np.random.RandomState(0)
    n, rps, c, K = 7, 5, 6, 4
    x, dy = rs.randn(n, rps, c).astype(np.float32), rs.randn(n, rps, c).astype(np.float32)
    gamma, beta = rs.randn(K, c).astype(np.float32), rs.randn(K, c).astype(np.float32)
    labels = rs.randint(K, size=n)
    mask = np.where(rs.rand(n, rps, c) < 0.5, 1.0, 0.2)
    y0, dx0, dg0, db0 = M._bn_ref(x, labels, gamma, beta, dy, mask)
    r = E.bn_ref(x, labels, gamma, beta)
    dx, dg, db = E.bn_ref_bwd(r, dy, mask, K)
    for a, b in ((r.pre, y0), (dx, dx0), (dg, dg0), (db, db0)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert E.mask_of(E.ACT_LRELU, np.array([-1.0, 0.0, 2.0])).tolist() == [0.2, 0.2, 1.0] and E.mask_of(E.ACT_RELU, np.array([-1.0, 0.0, 2.0])).tolist() == [0, 0, 1]
    assert E.act_ref(E.ACT_LRELU, np.array([-1.0, 2.0])).tolist() == [-0.2, 2.0]


def test_row_and_channel_scales():
    """assert_rows_close scales every row by itself: an error that the tensor's max would hide fails, a zero row must be exactly zero."""
    ref = np.array([[1000.0, 2.0], [1e-3, 2e-3], [0.0, 0.0]])
    E.assert_rows_close(ref * (1 + 1e-6), ref, 2e-5, "ok")
    bad = ref.copy()
    bad[1, 0] += 1e-4                      # 1e-7 of the tensor's max, 5 % of the row's
    with pytest.raises(AssertionError):
        E.assert_rows_close(bad, ref, 2e-5, "small row")
    bad = ref.copy()
    bad[2, 1] = 1e-30
    with pytest.raises(AssertionError):
        E.assert_rows_close(bad, ref, 2e-5, "zero row")
    with pytest.raises(AssertionError):
        E.assert_channels_close(bad.T.reshape(1, 2, 3), ref.T.reshape(1, 2, 3), 2e-5, "zero channel")
