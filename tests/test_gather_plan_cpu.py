"""The launch decisions of the gather-GEMM family (csrc/gather_plan.h) swept without a GPU: tests/tools/gather_plan_sweep.cpp, built with
the host C++ compiler and -fsanitize=address,undefined, run as a child process -- nothing is loaded into this interpreter.

Checked: the invariants the program asserts over its grid, for the default switches and with each switch off (reduction chunks cover
[0, R) once and start on whole K-steps, the final chunk count never exceeds the planned one, slabs and column-sum partials fit the
workspace queries and do not overlap, at most 1024 partial rows on the doubling routes, the 8-wide column-sum kernel only where its row
lanes fill the 2048-float buffer, the K-group reduction area inside the launch's LDS, FastDiv::div(n) == n / d on the host branch, the
stride-2 parity classes partition pixels and taps); that every case of tests/test_gpu_gather_edges.py reaches the branch its table
names -- with the column-sum tail and without it, the label-column and graph-replay shapes included, and the tail's byte count as
the GPU file restates it; that the tables together reach every branch listed there."""
import os
import shutil
import subprocess

import pytest

from tests import test_gpu_gather_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "tools", "gather_plan_sweep.cpp")
HEADER = os.path.join(ROOT, "robust-conditional-gan_amd", "csrc", "gather_plan.h")


def _cxx():
    return next((p for p in (shutil.which(n) for n in (os.environ.get("CXX") or "c++", "g++", "clang++")) if p), None)


@pytest.fixture(scope="module")
def sweep_program(tmp_path_factory):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gather_plan") / "gather_plan_sweep")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # the sanitizer runtimes linked statically where the compiler offers it, dynamically otherwise
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if subprocess.run([cxx] + flags + static + ["-o", exe, SOURCE], capture_output=True).returncode == 0:
            return exe
    subprocess.run([cxx] + flags + ["-o", exe, SOURCE], check=True)      # (shows the compiler's message)


def _run(exe, mode, stdin=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("RCGAN_GG_", "RCGAN_NARROW_", "RCGAN_S2_"))}
    return subprocess.run([exe, mode], input=stdin, env=env, capture_output=True, text=True, timeout=600)


def test_header_compiles_with_the_host_compiler_alone():
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", HEADER, os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(HEADER) as fh:
        text = fh.read()
    assert "getenv" not in text and "hip/" not in text and "__global__" not in text


def test_invariants_hold_over_the_grid(sweep_program):
    r = _run(sweep_program, "sweep")
    assert r.returncode == 0 and "violations 0" in r.stdout and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    swept = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("swept ")]
    assert swept == ["default", "RCGAN_GG_KS=1", "RCGAN_GG_KS=2", "RCGAN_GG_KS_MINSTEPS=off", "RCGAN_GG_KS2_MINWGS=off", "RCGAN_GG_SPLIT_R=0",
                     "RCGAN_GG_WGRAD_FIT=0", "RCGAN_NARROW_TWO_STEP=0", "RCGAN_S2_LPT=0"], swept
    assert int(r.stdout.strip().splitlines()[-1].split()[1]) > 50000000, r.stdout[-200:]


def _fields(line):
    return dict(f.split("=", 1) for f in line.split()[2:] if "=" in f)


def test_edge_cases_reach_the_branches_they_name(sweep_program):
    claims = E.plan_claims()
    r = _run(sweep_program, "cases", "\n".join(line for _, line, _ in claims) + "\n")
    assert r.returncode == 0 and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("case ")]
    assert len(lines) == len(claims)
    reached = {}
    wrong = []
    for (name, line, expect), got in zip(claims, lines):
        f = _fields(got)
        for k, v in expect.items():
            if not E.matches(f[k], v):
                wrong.append("%s (%s): %s is %s, the table says %s" % (name, line, k, f[k], v))
        if line.split()[1] == "f32":
            for op, branch in f.items():
                for want in E.BRANCHES:
                    if want[0] == op and E.matches(branch, want[1]):
                        reached.setdefault(want, []).append(name)
    assert not wrong, "\n".join(wrong)
    for want in E.BRANCHES:
        print("%-6s %-44s %s" % (want[0], want[1], ", ".join(reached.get(want, [])[:3]) or "-- NOT REACHED --"))
    missing = [b for b in E.BRANCHES if b not in reached]
    assert not missing, missing
    # the 16-bit contexts never split a reduction and never take the two-step route
    for (name, line, _), got in zip(claims, lines):
        if line.split()[1] == "h16":
            assert "split" not in got and "two_step" not in got, got
