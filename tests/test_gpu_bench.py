"""bench.py on the device: --steps sets the timed iterations, the JSON line carries ms_per_step, and --dump-outputs writes what the
last timed iteration left (costs, variables, spectral-norm u vectors) consistent with the line's own losses."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_and_dump_outputs(tmp_path):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import create_variables
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--no-cpu-baseline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["config"]["losses_finite"]
    gs, ds, cs, U = create_variables(0, "rcgan")
    want = {"d_loss", "g_loss"} | {"param." + n.replace("/", ".") for n, _, _ in gs + ds + cs} | \
        {"sn_u." + k.replace("/", ".") for k in U}
    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(out)}
    assert set(got) == want
    assert line["dump_outputs"]["arrays"] == len(want)
    assert sum(v.nbytes for v in got.values()) == line["dump_outputs"]["bytes"] <= 64 << 20
    for k, v in got.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    for n, _, v in gs + ds + cs:
        assert got["param." + n.replace("/", ".")].shape == v.shape, n
    assert round(float(got["d_loss"][0]), 4) == line["config"]["d_loss"]
    assert round(float(got["g_loss"][0]), 4) == line["config"]["g_loss"]
