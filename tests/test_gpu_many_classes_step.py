"""Whole steps of a 100-class CIFAR RCGAN (CifarRCGAN(n_classes=100): CIFAR-100's fine labels) on the GPU: parity with the numpy
oracle in float64 at the tolerances of test_gpu_cifar_step.py, the embedding property against a 10-class model, graph replay,
checkpoints and a short run of the trainer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cifar as oc
from tests import test_gpu_cifar_step as base

pytestmark = pytest.mark.gpu

K = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c(alpha=0.6, k=K):
    from rcgan_amd.cifar import C_ALPHA
    return C_ALPHA(alpha, k)


def _batches(rs, B, k=K, hi=None):
    hi = hi or k
    C = _c(0.6, k)
    Cinv = np.linalg.inv(C)
    lab = rs.randint(hi, size=B)
    raw = dict(images=rs.randint(0, 256, size=(B, 3072)), noise=rs.uniform(0, 1 / 128., size=(B, 3072)).astype(np.float32),
               labels=lab, labels_random=rs.randint(hi, size=B), labels_biased=rs.randint(hi, size=B),
               inv_weights=Cinv[lab].astype(np.float32), z=rs.randn(B, 128).astype(np.float32))
    g = dict(labels_random_G=rs.randint(hi, size=2 * B), labels_biased_G=rs.randint(hi, size=2 * B),
             z_G=rs.randn(2 * B, 128).astype(np.float32))
    return C, raw, g


def _variables(alg, perm, k=K):
    from rcgan_amd.cifar import create_variables
    gs, ds, cs, U = create_variables(0, alg, perm, "linear", True, 0.2, n_classes=k)
    rs = np.random.RandomState(3)

    def jitter(specs):
        out = []
        for n, shp, v in specs:
            if n.endswith("/Biases") or n.endswith("/b") or "CondBatchNorm" in n:
                v = (v + 0.1 * rs.randn(*shp)).astype(np.float32)
            out.append((n, shp, v))
        return out
    return jitter(gs), jitter(ds), cs, U


def _make(alg, perm, B, dtype, variables, use_graphs=False, k=K):
    from rcgan_amd.cifar import CifarRCGAN
    return CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype=dtype, perm_classifier=perm, perm_multiplier=1.0,
                      use_graphs=use_graphs, device_rng=False, variables=variables, arena_bytes=2 << 30, n_classes=k)


def test_oracle_reads_vocab_at_call_time():
    import inspect
    src = inspect.getsource(oc)
    assert "def c_alpha" in src and "VOCAB = 10" in src
    # every other use of VOCAB sits inside a function body (module level: only its definition)
    top = [ln for ln in src.splitlines() if "VOCAB" in ln and not ln.startswith((" ", "\t"))]
    assert top == ["VOCAB = 10"], top


@pytest.mark.parametrize("alg,perm", [("rcgan", False), ("rcgan-u", True), ("biased", False), ("unbiased", False)])
def test_step_parity_100_classes(alg, perm, monkeypatch):
    monkeypatch.setattr(oc, "VOCAB", K)
    rs = np.random.RandomState(41)
    B = 4
    C, raw, gb = _batches(rs, B)
    variables = _variables(alg, perm)
    m = _make(alg, perm, B, "f32", variables)
    P = {n: v.copy() for n, _, v in variables[0] + variables[1] + variables[2]}
    Uo = {k: v.copy() for k, v in variables[3].items()}
    monkeypatch.setattr(base, "m_init", {k: v.copy() for k, v in P.items()})
    try:
        assert m.get_params()["Discriminator/Embedding.Label/embedding_map"].shape == (K, 300)
        base._check(m, P, Uo, alg, perm, raw, gb, C, "f32")
    finally:
        m.ctx.close()


def test_embedding_property_against_ten_classes():
    """A 100-class model whose batches use classes 0..9 only, with table rows 0..9 (every class-indexed table) equal to a
    10-class model's and a block-diagonal C: the same losses and, for the shared rows, the same gradients; rows 10..99 get
    exact zeros."""
    rs = np.random.RandomState(43)
    B = 4
    C10, raw, gb = _batches(rs, B, k=10)
    v10 = _variables("rcgan", False, 10)
    v100 = _variables("rcgan", False, K)
    p10 = {n: v for n, _, v in v10[0] + v10[1]}

    def widen(specs):
        out = []
        for n, shp, v in specs:
            if shp[0] == K and n in p10 and p10[n].shape[0] == 10:
                v = v.copy()
                v[:10] = p10[n]
            else:
                v = p10[n].copy() if n in p10 and p10[n].shape == v.shape else v
            out.append((n, shp, v))
        return out
    v100 = (widen(v100[0]), widen(v100[1]), v100[2], dict(v10[3]))
    C100 = np.eye(K)
    C100[:10, :10] = C10
    res = []
    for k, variables, C in ((10, v10, C10), (K, v100, C100)):
        m = _make("rcgan", False, B, "f32", variables, k=k)
        try:
            m.ctx.view(m.inp["C_const"]).copy_(__import__("torch").from_numpy(C.astype(np.float32)))
            inv = np.linalg.inv(C)[raw["labels"]].astype(np.float32)
            m.set_inputs(labels_all=base._labels_all("rcgan", raw), **dict(raw, inv_weights=inv))
            m.d_step(iteration=0)
            d_loss, _ = m.losses()
            gd = m.get_grads(m.PD)
            m.set_inputs(**gb)
            m.g_step(iteration=1)
            _, g_loss = m.losses()
            res.append((d_loss, g_loss, gd, m.get_grads(m.PG)))
        finally:
            m.ctx.close()
    (d10, g10, gd10, gg10), (d100, g100, gd100, gg100) = res
    assert abs(d10 - d100) <= 2e-5 * max(1.0, abs(d10)) and abs(g10 - g100) <= 2e-5 * max(1.0, abs(g10)), (d10, d100, g10, g100)
    for a, b in ((gd10, gd100), (gg10, gg100)):
        # (floor: conv biases feeding a batch norm have an exactly-zero true gradient, test_gpu_cifar_step.py)
        gmax = max(float(np.abs(g).max()) for g in a.values())
        for n, g in a.items():
            h = b[n]
            if h.shape != g.shape:
                assert (h[10:] == 0).all(), "rows 10..99 of %s" % n
                h = h[:10]
            scale = max(float(np.abs(g).max()), 1e-3 * gmax)
            assert float(np.abs(h - g).max()) <= 2e-3 * scale, n


def _step_inputs(m, rs, B):
    C, raw, gb = _batches(rs, B)
    m.set_inputs(labels_all=base._labels_all("rcgan-u", raw), **raw)
    return raw, gb


def test_graph_replay_is_bitwise_at_100_classes():
    """d_step / g_step replayed from captured graphs give the bits of eager steps."""
    alg, B = "rcgan-u", 8
    variables = _variables(alg, True)
    outs = {}
    for graphs in (False, True):
        m = _make(alg, True, B, "bf16", variables, use_graphs=graphs)
        rs = np.random.RandomState(44)
        try:
            trace = []
            for it in range(3):
                raw, gb = _step_inputs(m, rs, B)
                m.d_step(iteration=it)
                trace.append(m.losses()[0])
                m.set_inputs(**gb)
                m.g_step(iteration=it)
                trace.append(m.losses()[1])
            outs[graphs] = (trace, m.get_params())
        finally:
            m.ctx.close()
    assert outs[False][0] == outs[True][0]
    for k, v in outs[False][1].items():
        assert np.array_equal(v, outs[True][1][k]), k


def test_critic_steps_graph_equals_five_d_steps_at_100_classes(monkeypatch):
    """critic_steps as one captured graph == five d_step calls (RCGAN_CRITIC_GRAPH=0), bit for bit."""
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    alg, B = "rcgan-u", 8
    rs = np.random.RandomState(45)
    ds = []
    for _ in range(N_CRITIC):
        raw = _batches(rs, B)[1]
        d = {k: raw[k] for k in ("images", "labels", "labels_random", "labels_biased", "inv_weights")}
        d["labels_all"] = base._labels_all(alg, raw)
        ds.append(d)
    outs = []
    for one_graph in ("1", "0"):
        monkeypatch.setenv("RCGAN_CRITIC_GRAPH", one_graph)
        m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=5, perm_classifier=True, confuse_init=True,
                       use_graphs=True, device_rng=True, arena_bytes=2 << 30, n_classes=K)
        try:
            m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
            m.prepare_critic_fakes()
            assert m._critic_graph_ok() == (one_graph == "1")
            if one_graph == "1":
                m.critic_steps(ds, iteration=0)
            else:
                for d in ds:
                    m.feed_host("d", **d)
                    m.d_step(iteration=0)
            outs.append(m.get_params())
        finally:
            m.ctx.close()
    for k, v in outs[0].items():
        assert np.array_equal(v, outs[1][k]), k


def test_checkpoint_round_trip_and_class_count_check(tmp_path):
    from rcgan_amd.cifar import CifarRCGAN
    B = 4
    variables = _variables("rcgan", False)
    m = _make("rcgan", False, B, "bf16", variables)
    try:
        raw, gb = _step_inputs(m, np.random.RandomState(46), B)
        m.d_step(iteration=0)
        sd = m.state_dict()
        assert sd["Generator/G.Block.1.N1/CondBatchNorm/scale"].shape == (K, 1024)
        m2 = _make("rcgan", False, B, "bf16", _variables("rcgan", False))
        try:
            m2.load_state_dict(sd)
            for k, v in m.get_params().items():
                assert np.array_equal(v, m2.get_params()[k]), k
        finally:
            m2.ctx.close()
    finally:
        m.ctx.close()
    m10 = CifarRCGAN(algorithm="rcgan", batch_size=B, dtype="bf16", use_graphs=False, device_rng=False, arena_bytes=1 << 30)
    try:
        sd10 = m10.state_dict()
    finally:
        m10.ctx.close()
    m3 = _make("rcgan", False, B, "bf16", _variables("rcgan", False))
    try:
        with pytest.raises(ValueError, match="checkpoint has 10 classes, this model has 100"):
            m3.load_state_dict(sd10)
    finally:
        m3.ctx.close()


def test_trainer_cifar100_synthetic(tmp_path):
    log = tmp_path / "train.log"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "rcgan_amd.train_cifar", "--dataset", "cifar100", "--synthetic", "--synthetic_kind", "templates",
           "--niters", "20", "--batch_size", "16", "--log_file", str(log), "--parent_dir", str(tmp_path), "--expt_dir", "run",
           "--inception_freq", "0", "--sample_freq", "1000000", "--generated_label_accuracy_freq", "10"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    text = log.read_text()
    assert "100 classes" in text and "skipped" in text
    from rcgan_amd.host import latest_checkpoint, load_checkpoint
    sd = load_checkpoint(latest_checkpoint(str(tmp_path / "run" / "checkpoint")))
    assert sd["Generator/G.OutputNorm/CondBatchNorm/offset"].shape == (K, 256)
    assert sd["Discriminator/Embedding.Label/embedding_map"].shape == (K, 300)
    costs = [float(part.split(":")[1]) for ln in text.splitlines() for part in ln.split(", ") if part.split(":")[0].strip() in ("d_cost", "g_cost")]
    assert costs and np.isfinite(costs).all(), text[-2000:]
