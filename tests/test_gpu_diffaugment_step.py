"""CifarRCGAN(diffaugment=...): whole steps with the augmentation between the images and the critic.

* one critic step and one generator step, fp32, against float64 autograd of oracle.torch_port.CifarTorch with the restated
  augmentation (tests/diffaugment_ref.py) in front of its discriminator, the same explicit draws on both sides;
* the five critic steps as one captured graph against five d_step() calls, bit for bit, with fresh draws on every replay;
* the option off is the engine it was; the draws leave the noise / z stream alone; K = 20, fp16 and the other routes run.
"""
import numpy as np
import pytest
import torch

from oracle import cifar as oc
from tests import diffaugment_ref as R
from tests.gpu_util import rel_err

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"


def _batch(rs, B, K=10, alpha=0.6):
    C = (1 - alpha) / (K - 1) * np.ones((K, K)) + (alpha - (1 - alpha) / (K - 1)) * np.eye(K)
    lab = rs.randint(K, size=B)
    raw = dict(images=rs.randint(0, 256, size=(B, 3072)), labels=lab, labels_random=rs.randint(K, size=B),
               labels_biased=rs.randint(K, size=B), inv_weights=np.linalg.inv(C)[lab].astype(np.float32))
    return C, raw


def _labels_all(alg, raw):
    return np.concatenate([raw["labels"], raw["labels_random"] if alg in ("biased", "unbiased") else raw["labels_biased"]])


def _host_draws(rs, B):
    """What the host supplies with device_rng=False: noise, z and one row of u per image the critic sees."""
    u = lambda n: np.minimum(rs.uniform(size=(n, 8)).astype(np.float32), np.float32(R.U_MAX))
    d = dict(noise=rs.uniform(0, 1 / 128., size=(B, 3072)).astype(np.float32), z=rs.randn(B, 128).astype(np.float32), aug_u=u(2 * B))
    g = dict(z_G=rs.randn(2 * B, 128).astype(np.float32), aug_u_G=u(2 * B))
    return d, g


def _jittered_variables(alg="rcgan"):
    from rcgan_amd.cifar import create_variables
    gs, ds, cs, U = create_variables(0, alg, False, "linear", True, 0.2)
    rs = np.random.RandomState(3)

    def jitter(specs):      # de-trivialise the zero-initialised tensors (biases, condBN tables) so their gradients matter
        out = []
        for n, shp, v in specs:
            if n.endswith("/Biases") or n.endswith("/b") or "CondBatchNorm" in n:
                v = (v + 0.1 * rs.randn(*shp)).astype(np.float32)
            out.append((n, shp, v))
        return out
    return jitter(gs), jitter(ds), cs, U


def _compare(tag, got, grads, tol):
    """Every gradient tensor within ``tol`` norm-relative.  A tensor whose true gradient is zero (a convolution bias in front of a
    batch norm; largest reference entry below 1e-3 of the step's largest) has no norm to relate to: its entries stay under half that
    floor, the rule of tests/test_gpu_fullbatch_steps.py."""
    gmax = max(float(np.abs(g).max()) for g in grads.values())
    floor, bad = 1e-3 * gmax, []
    for k, gref in grads.items():
        a = got[k]
        assert np.isfinite(a).all(), k
        if float(np.abs(gref).max()) > floor:
            e = rel_err(a, gref)
            print("%s %-60s norm-rel %.3e" % (tag, k, e))
            if e > tol:
                bad.append("%s %s: norm-rel %.3e > %.1e" % (tag, k, e, tol))
        else:
            e = float(np.abs(a - gref).max()) / floor
            print("%s %-60s %.3e of the zero-gradient floor" % (tag, k, e))
            if e > 0.5:
                bad.append("%s %s: %.3e of the floor" % (tag, k, e))
    assert not bad, "\n".join(bad)


def test_critic_and_generator_step_against_float64():
    """fp32, rcgan, B = 8, all three augmentations, the draws fed from the host.  Bound: 2e-3 norm-relative per gradient tensor, what
    DESIGN 4 records for the fp32 whole iteration against the float64 oracle.  Seed 31: every hinge argument of the critic step is
    further than 1e-3 from its kink (asserted below), so no term can take the other branch under fp32 rounding."""
    import rcgan_amd  # noqa: F401
    from oracle.torch_port import CifarTorch
    from rcgan_amd.cifar import CifarRCGAN

    class AugTorch(CifarTorch):
        """CifarTorch with the augmentation in front of the discriminator; perm (not used here) would see the plain images."""
        aug_u, policy = None, 7

        def discriminator(self, x, update):
            x = R.diffaugment(x.reshape(-1, 32, 32, 3), self.aug_u, self.policy).reshape(-1, 3072)
            return super().discriminator(x, update)

    B, alg = 8, "rcgan"
    rs = np.random.RandomState(31)
    C, raw = _batch(rs, B)
    dd, gd = _host_draws(rs, B)
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    variables = _jittered_variables(alg)
    P = {n: v.copy() for n, _, v in variables[0] + variables[1]}
    U = {k: v.copy() for k, v in variables[3].items()}
    cfg = dict(algorithm=alg, C=C)
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="f32", use_graphs=False, device_rng=False, variables=variables,
                   arena_bytes=2 << 30, diffaugment=FULL)
    try:
        assert m.aug == 7 and m.inp["aug_u"].shape == (2 * B, 8) and m.inp["aug_u_G"].shape == (2 * B, 8)
        assert "aug_u" in [f[0] for f in m.feed_layout["d"]] and "aug_u_G" in [f[0] for f in m.feed_layout["g"]]
        # ---- critic step
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        net = AugTorch(P, U, torch.float64)
        net.aug_u = dd["aug_u"]
        cost = net.disc_cost(cfg, dict(real=oc.preprocess_real(raw["images"], dd["noise"]), z=dd["z"], **raw))
        names = [k for k in net.P if k.startswith("Discriminator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        kink = min(float(t.abs().min()) for t in net.hinge_args.values())
        active = sum(int((t > 0).sum()) for t in net.hinge_args.values())
        print("hinge arguments: nearest to the kink %.3e, %d of %d active" % (kink, active, 2 * B))
        assert kink > 1e-3 and active > 0, "a hinge term sits at its kink (or none is active) at this seed: pick another"
        d_loss, _ = m.losses()
        assert abs(d_loss - float(cost.detach())) <= 2e-5 * max(1.0, abs(float(cost.detach()))), (d_loss, float(cost.detach()))
        _compare("D", m.get_grads(m.PD), grads, 2e-3)
        # ---- generator step, from the device's own weights and spectral-norm state after the critic update
        P2, U2 = m.get_params(), m.get_state()
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=1)
        net = AugTorch(P2, U2, torch.float64)
        net.aug_u = gd["aug_u_G"]
        cost = net.gen_cost(cfg, dict(z=gd["z_G"], **gb))
        names = [k for k in net.P if k.startswith("Generator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        _, g_loss = m.losses()
        assert abs(g_loss - float(cost.detach())) <= 2e-5 * max(1.0, abs(float(cost.detach()))), (g_loss, float(cost.detach()))
        _compare("G", m.get_grads(m.PG), grads, 2e-3)
    finally:
        m.ctx.close()


def _iterations(rs, B, n_it, alg="rcgan", K=10):
    from rcgan_amd.cifar import N_CRITIC
    its = []
    for _ in range(n_it):
        ds = []
        for _ in range(N_CRITIC):
            raw = _batch(rs, B, K)[1]
            raw["labels_all"] = _labels_all(alg, raw)
            ds.append(raw)
        its.append((ds, dict(labels_random_G=rs.randint(K, size=2 * B), labels_biased_G=rs.randint(K, size=2 * B))))
    return its


def _iterate(m, ds, g, it, one_graph):
    m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
    m.prepare_critic_fakes()
    if one_graph:
        m.critic_steps(ds, iteration=it)
    else:
        for d in ds:
            m.feed_host("d", **d)
            m.d_step(iteration=it)
    m.feed_host("g", **g)
    m.g_step(iteration=it)


def test_critic_steps_as_one_graph_equal_single_steps_and_draw_afresh(monkeypatch):
    """bf16, draws on the device, B = 8 (the batch of the one-graph test in tests/test_gpu_cifar_step.py): critic_steps() as one
    captured graph -- run once eagerly, then replayed twice -- against d_step() calls from the same state, the option on."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B = 8
    its = _iterations(np.random.RandomState(23), B, 3)
    outs = []
    for one_graph in (True, False):
        monkeypatch.setenv("RCGAN_CRITIC_GRAPH", "1" if one_graph else "0")
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=5, use_graphs=True, device_rng=True,
                       arena_bytes=2 << 30, diffaugment=FULL)
        try:
            assert "aug_u" not in [f[0] for f in m.feed_layout["d"]]      # drawn on the device: not a field of the feed
            us, crit = [], []
            for it, (ds, g) in enumerate(its):
                m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
                m.prepare_critic_fakes()
                assert m._critic_graph_ok() == one_graph
                if one_graph:
                    m.critic_steps(ds, iteration=it * 9000)
                else:
                    for d in ds:
                        m.feed_host("d", **d)
                        m.d_step(iteration=it * 9000)
                us.append(m.ctx.download(m.inp["aug_u"]).copy())           # the draws of the last critic step of this iteration
                crit.append({n: m.PD.get(n) for n in m.PD.names})
                m.feed_host("g", **g)
                m.g_step(iteration=it * 9000)
                us.append(m.ctx.download(m.inp["aug_u_G"]).copy())
            assert ("d5" in m._graphs) == one_graph
            outs.append((us, crit, m.get_params(), m.get_state()))
        finally:
            m.ctx.close()
    (ua, ca, pa, sa), (ub, cb, pb, sb) = outs
    for i, (a, b) in enumerate(zip(ua, ub)):
        assert np.array_equal(a, b), "draw %d differs between the two forms" % i
        assert (a >= 0).all() and (a < 1).all()
    # iteration 0 ran eagerly (and was captured), iterations 1 and 2 are replays: each drew other numbers
    for i in range(len(ua)):
        for j in range(i + 1, len(ua)):
            assert not np.array_equal(ua[i], ua[j]), "draws %d and %d are the same numbers" % (i, j)
    for it in range(3):
        for k in ca[it]:
            assert np.array_equal(ca[it][k], cb[it][k]), "critic weights after iteration %d: %s" % (it, k)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_option_off_is_the_engine_it_was():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B = 8
    rs = np.random.RandomState(4)
    _, raw = _batch(rs, B)
    dd, gd = _host_draws(rs, B)
    dd.pop("aug_u")
    gd.pop("aug_u_G")
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    outs = []
    for kw in (dict(diffaugment=""), dict()):
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=False,
                       arena_bytes=2 << 30, **kw)
        try:
            assert m.aug == 0 and m.aug_rng_state is None
            assert "aug_u" not in m.inp and "aug_u_G" not in m.inp
            assert all(f[0] not in ("aug_u", "aug_u_G") for fields in m.feed_layout.values() for f in fields)
            m.set_inputs(labels_all=_labels_all("rcgan", raw), **raw, **dd)
            m.d_step(iteration=0)
            m.set_inputs(**gb, **gd)
            m.g_step(iteration=0)
            outs.append((m.get_params(), m.losses()))
        finally:
            m.ctx.close()
    (pa, la), (pb, lb) = outs
    assert la == lb
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def test_the_draws_have_a_stream_of_their_own():
    """One iteration with the draws on the device: the noise / z stream ends at the same position with the option on and off, and
    the generator's z of the iteration is the same numbers."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B = 8
    (ds, g), = _iterations(np.random.RandomState(9), B, 1)
    seen = []
    for policy in (FULL, ""):
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=7, use_graphs=False, device_rng=True,
                       arena_bytes=2 << 30, diffaugment=policy)
        try:
            _iterate(m, ds, g, 0, one_graph=True)
            m.ctx.sync()
            seen.append((m.rng_state.cpu().numpy().copy(), m.ctx.download(m.inp["z_G"]).copy(), m.ctx.download(m.inp["z_all"]).copy(),
                         None if m.aug_rng_state is None else m.aug_rng_state.cpu().numpy().copy()))
        finally:
            m.ctx.close()
    (ra, zga, zaa, aug_on), (rb, zgb, zab, aug_off) = seen
    assert ra[0] > 0 and np.array_equal(ra, rb), (ra, rb)
    assert np.array_equal(zga, zgb) and np.array_equal(zaa, zab)
    # six draws of 2B rows of eight, four numbers to a counter
    assert aug_off is None and int(aug_on[0]) == 6 * (2 * B * 8 // 4)


def _one_critic_step(dtype, K, alg="rcgan", **kw):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B = 8
    rs = np.random.RandomState(12)
    _, raw = _batch(rs, B, K)
    dd, _ = _host_draws(rs, B)
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype=dtype, seed=1, use_graphs=False, device_rng=False, n_classes=K,
                   arena_bytes=2 << 30, diffaugment=FULL, **kw)
    try:
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        d_loss, _ = m.losses()
        grads = m.get_grads(m.PD)
        assert np.isfinite(d_loss)
        for k, gk in grads.items():
            assert np.isfinite(gk).all(), k
        assert float(np.abs(grads["Discriminator/D.Block.1.Conv1/Filters"]).max()) > 0
        assert float(np.abs(grads["Discriminator/D.Block.1.Shortcut/Filters"]).max()) > 0
    finally:
        m.ctx.close()


def test_critic_step_with_twenty_classes_bf16():
    _one_critic_step("bf16", 20)


def test_critic_step_fp16():
    _one_critic_step("f16", 10)


@pytest.mark.parametrize("alg,env", [("rcgan-u", {}), ("unbiased", {"RCGAN_FUSED_HEAD": "0"}), ("biased", {"RCGAN_RIDE_INPUTS": "0"}),
                                     ("rcgan-u", {"RCGAN_FUSED_HEAD": "0"})])
def test_one_iteration_on_the_other_routes(alg, env, monkeypatch):
    """The other algorithms, the op-by-op head and the step without the input rider: an iteration with the draws on the device runs,
    with finite losses and gradients that reach the generator through the adjoint."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 8
    (ds, g), = _iterations(np.random.RandomState(5), B, 1, alg)
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=3, use_graphs=False, device_rng=True, perm_classifier=True,
                   arena_bytes=2 << 30, diffaugment=FULL)
    try:
        _iterate(m, ds, g, 0, one_graph=True)
        d_loss, g_loss = m.losses()
        assert np.isfinite(d_loss) and np.isfinite(g_loss)
        gg = m.get_grads(m.PG)
        for k, gk in gg.items():
            assert np.isfinite(gk).all(), k
        assert float(np.abs(gg["Generator/G.Output/Filters"]).max()) > 0
    finally:
        m.ctx.close()
