"""CifarRCGAN(diffaugment=..., ada_target=...): whole steps with the adaptive augmentation probability.

(a) one critic step and one generator step, fp32, against float64 autograd of oracle.torch_port.CifarTorch with the restated GATED
    augmentation (tests/ada_ref.py) in front of its discriminator -- per sample it is the same affine family as the ungated one, so
    the bounds are those of test_gpu_diffaugment_step.test_critic_and_generator_step_against_float64;
(b) p pinned at 1: bit-identical to the plain diffaugment engine fed the same draws;
(c) the five critic steps as one captured graph against five d_step() calls: weights AND controller state bit for bit, and the state
    after every single step is the float32 reference applied to the logits that step left behind;
(d) the other algorithms and the unfused head; (e) the checkpoint round trip; (f) the option off is the engine it was.
"""
import collections

import numpy as np
import pytest
import torch

from oracle import cifar as oc
from tests import ada_ref as A
from tests import diffaugment_ref as R
from tests.test_gpu_diffaugment_step import (FULL, _batch, _compare, _host_draws, _iterations, _jittered_variables, _labels_all)

pytestmark = pytest.mark.gpu

NEW = ("rcgan_diffaugment_gated_fwd", "rcgan_diffaugment_sampled_bwd", "rcgan_ada_update")
SEED_A = 31


def _gates(rs, n):
    return np.minimum(rs.uniform(size=(n, 4)).astype(np.float32), np.float32(R.U_MAX))


def _host_draws_ada(rs, B):
    d, g = _host_draws(rs, B)
    d["aug_gate"], g["aug_gate_G"] = _gates(rs, 2 * B), _gates(rs, 2 * B)
    return d, g


def _ada_torch():
    from oracle.torch_port import CifarTorch

    class AdaTorch(CifarTorch):
        """CifarTorch with the gated augmentation in front of the discriminator."""
        aug_u = aug_gate = None
        p, policy = 0.5, 7

        def discriminator(self, x, update):
            x = A.diffaugment(x.reshape(-1, 32, 32, 3), self.aug_u, self.aug_gate, self.p, self.policy).reshape(-1, 3072)
            return super().discriminator(x, update)
    return AdaTorch


def oracle_inputs(seed, B=8, alg="rcgan"):
    """Everything test (a) feeds, from one seed (also what a seed search without a GPU evaluates)."""
    rs = np.random.RandomState(seed)
    C, raw = _batch(rs, B)
    dd, gd = _host_draws_ada(rs, B)
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    return C, raw, dd, gd, gb, _jittered_variables(alg)


def oracle_critic(C, raw, dd, P, U, alg="rcgan", p=0.5):
    net = _ada_torch()(P, U, torch.float64)
    net.aug_u, net.aug_gate, net.p = dd["aug_u"], dd["aug_gate"], p
    cost = net.disc_cost(dict(algorithm=alg, C=C), dict(real=oc.preprocess_real(raw["images"], dd["noise"]), z=dd["z"], **raw))
    return net, cost


def test_critic_and_generator_step_against_float64():
    """fp32, rcgan, B = 8, all three augmentations gated at p = 0.5, draws and gates fed from the host; ada_images is so large that
    the update (which runs: interval 1) cannot move p in fp32.  Bounds: 2e-3 norm-relative per gradient tensor and 2e-5 on the
    losses, those of the ungated test.  The seed keeps every hinge argument of the critic step further than 1e-3 from its kink
    (asserted below)."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B, alg, p = 8, "rcgan", 0.5
    C, raw, dd, gd, gb, variables = oracle_inputs(SEED_A, B, alg)
    P = {n: v.copy() for n, _, v in variables[0] + variables[1]}
    U = {k: v.copy() for k, v in variables[3].items()}
    cfg = dict(algorithm=alg, C=C)
    pol_d, pol_g = A.sample_policy(dd["aug_gate"], p, 7), A.sample_policy(gd["aug_gate_G"], p, 7)
    assert len(set(pol_d.tolist())) >= 5 and len(set(pol_g.tolist())) >= 5, "the gates of this seed exercise few policies"
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="f32", use_graphs=False, device_rng=False, variables=variables,
                   arena_bytes=2 << 30, diffaugment=FULL, ada_target=0.6, ada_images=1e12, ada_interval=1, ada_p_init=p)
    try:
        assert m.ada and m.inp["aug_gate"].shape == (2 * B, 4) and m.inp["aug_gate_G"].shape == (2 * B, 4)
        assert [f[0] for f in m.feed_layout["d"]][-2:] == ["aug_u", "aug_gate"] and [f[0] for f in m.feed_layout["g"]][-2:] == ["aug_u_G", "aug_gate_G"]
        assert m.inp["aug_u"].shape == (2 * B, 8)
        # ---- critic step
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        net, cost = oracle_critic(C, raw, dd, P, U, alg, p)
        names = [k for k in net.P if k.startswith("Discriminator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        kink = min(float(t.abs().min()) for t in net.hinge_args.values())
        active = sum(int((t > 0).sum()) for t in net.hinge_args.values())
        print("hinge arguments: nearest to the kink %.3e, %d of %d active" % (kink, active, 2 * B))
        assert kink > 1e-3 and active > 0, "a hinge term sits at its kink (or none is active) at this seed: pick another"
        d_loss, _ = m.losses()
        assert abs(d_loss - float(cost.detach())) <= 2e-5 * max(1.0, abs(float(cost.detach()))), (d_loss, float(cost.detach()))
        _compare("D", m.get_grads(m.PD), grads, 2e-3)
        # the controller ran once on the real rows and could not move p
        rep = m.ada_report()
        lg = m.ctx.download(m.ada_logits)[:B]
        want = A.update(A.new_state(p), lg, raw["labels"], 0.6, 1e12, 1)
        assert rep == dict(p=0.5, r_last=float(want[4]), updates=1), (rep, want)
        assert np.array_equal(m.ada_state.cpu().numpy(), want)
        # ---- generator step, from the device's own weights and spectral-norm state after the critic update
        P2, U2 = m.get_params(), m.get_state()
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=1)
        net = _ada_torch()(P2, U2, torch.float64)
        net.aug_u, net.aug_gate, net.p = gd["aug_u_G"], gd["aug_gate_G"], p
        cost = net.gen_cost(cfg, dict(z=gd["z_G"], **gb))
        names = [k for k in net.P if k.startswith("Generator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        _, g_loss = m.losses()
        assert abs(g_loss - float(cost.detach())) <= 2e-5 * max(1.0, abs(float(cost.detach()))), (g_loss, float(cost.detach()))
        _compare("G", m.get_grads(m.PG), grads, 2e-3)
        assert np.array_equal(m.ada_state.cpu().numpy(), want), "the generator step reads p and never updates it"
    finally:
        m.ctx.close()


def test_p_pinned_at_one_is_the_plain_diffaugment_engine():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B, alg = 8, "rcgan"
    rs = np.random.RandomState(41)
    rounds = []
    for _ in range(2):
        _, raw = _batch(rs, B)
        dd, gd = _host_draws_ada(rs, B)
        dd["aug_gate"][0, :] = R.U_MAX                      # the largest gate a draw can give still passes p = 1
        rounds.append((raw, dd, gd, dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))))
    outs = []
    for ada in (True, False):
        kw = dict(ada_target=-0.999, ada_interval=1, ada_p_init=1.0) if ada else {}
        m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=False,
                       arena_bytes=2 << 30, diffaugment=FULL, **kw)
        try:
            got = []
            for it, (raw, dd, gd, gb) in enumerate(rounds):
                drop = (lambda d: d) if ada else (lambda d: {k: v for k, v in d.items() if not k.startswith("aug_gate")})
                m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **drop(dd))
                m.d_step(iteration=it)
                m.ctx.sync()
                got.append((m.losses()[0], m.PD.grad.cpu().numpy().copy()))
                m.set_inputs(**gb, **drop(gd))
                m.g_step(iteration=it)
                m.ctx.sync()
                got.append((m.losses()[1], m.PG.grad.cpu().numpy().copy()))
            if ada:
                rep = m.ada_report()
                assert rep["p"] == 1.0 and rep["updates"] == 2 and -1.0 <= rep["r_last"] <= 1.0, rep
            outs.append((got, m.get_params()))
        finally:
            m.ctx.close()
    (ga, pa), (gb_, pb) = outs
    for i, ((la, sa), (lb, sb)) in enumerate(zip(ga, gb_)):
        assert la == lb, ("loss", i, la, lb)
        assert np.array_equal(sa.view(np.int32), sb.view(np.int32)), "gradient slab %d" % i
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def test_critic_steps_as_one_graph_equal_single_steps_with_a_moving_p(monkeypatch):
    """bf16, draws on the device, B = 8, ada_interval 2 and ada_images 64: p moves by 0.25 at the second and fourth critic step of
    every iteration, inside the captured graph, and the draws after it see it."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    B, target, images, interval = 8, 0.2, 64.0, 2
    its = _iterations(np.random.RandomState(23), B, 3)
    outs = []
    for one_graph in (True, False):
        monkeypatch.setenv("RCGAN_CRITIC_GRAPH", "1" if one_graph else "0")
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=5, use_graphs=True, device_rng=True,
                       arena_bytes=2 << 30, diffaugment=FULL, ada_target=target, ada_images=images, ada_interval=interval, ada_p_init=0.5)
        try:
            assert "aug_u" not in [f[0] for f in m.feed_layout["d"]] and "aug_gate" not in [f[0] for f in m.feed_layout["d"]]
            # u and its gates are one buffer, drawn by one launch
            assert m.inp["aug_gate"].ptr == m.inp["aug_u"].ptr + 4 * 2 * B * 8 and m._aug_draw["aug_u"].size == 2 * B * 12
            ref = A.new_state(0.5)
            states, crit, draws = [], [], []
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
                        m.ctx.sync()
                        # the controller after this step: the float32 reference on the logits the step's head left behind
                        ref = A.update(ref, m.ctx.download(m.ada_logits)[:B], d["labels"], target, images, interval)
                        got = m.ada_state.cpu().numpy()
                        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (it, got, ref)
                        # ... and the policies of the step's draw are the ones its p BEFORE the update gives
                m.ctx.sync()
                states.append(m.ada_state.cpu().numpy().copy())
                draws.append(m.ctx.download(m.inp["aug_gate"]).copy())
                crit.append({n: m.PD.get(n) for n in m.PD.names})
                m.feed_host("g", **g)
                m.g_step(iteration=it * 9000)
            assert ("d5" in m._graphs) == one_graph
            m.ctx.sync()
            # the stream position: six draws of 2B rows of twelve per iteration, four numbers to a counter -- no launch of its own for the gates
            assert int(m.aug_rng_state.cpu().numpy()[0]) == 3 * (N_CRITIC + 1) * (2 * B * 12 // 4)
            outs.append((states, crit, draws, m.get_params(), m.ada_report()))
        finally:
            m.ctx.close()
    (sa, ca, da, pa, ra), (sb, cb, db, pb, rb) = outs
    ps = [float(s[0]) for s in sb]
    print("p after each iteration:", ps, "report", rb)
    assert rb["updates"] == (3 * N_CRITIC) // interval and ra == rb
    assert len(set([0.5] + ps)) > 1, "p never moved"
    for it in range(3):
        assert np.array_equal(sa[it].view(np.int32), sb[it].view(np.int32)), ("ada_state after iteration %d" % it, sa[it], sb[it])
        assert np.array_equal(da[it], db[it]), "gates of iteration %d" % it
        for k in ca[it]:
            assert np.array_equal(ca[it][k], cb[it][k]), "critic weights after iteration %d: %s" % (it, k)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


@pytest.mark.parametrize("alg,env", [("rcgan-u", {}), ("unbiased", {"RCGAN_FUSED_HEAD": "0"}), ("biased", {"RCGAN_FUSED_HEAD": "0"}),
                                     ("rcgan-u", {"RCGAN_FUSED_HEAD": "0"}), ("unbiased", {}), ("biased", {"RCGAN_RIDE_INPUTS": "0"})])
def test_one_iteration_on_the_other_routes(alg, env, monkeypatch):
    """The other algorithms and the op-by-op head (every place the update reads its scores from): an iteration with the draws on the
    device runs, the controller counts every critic step, and what it computed is the reference on the real rows' scores."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, images = 8, 128.0
    (ds, g), = _iterations(np.random.RandomState(5), B, 1, alg)
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=3, use_graphs=False, device_rng=True, perm_classifier=True,
                   arena_bytes=2 << 30, diffaugment=FULL, ada_target=0.6, ada_images=images, ada_interval=N_CRITIC, ada_p_init=0.5)
    try:
        fused = env.get("RCGAN_FUSED_HEAD", "1") == "1"
        assert m.fused_head == fused and (m.ada_logits is not None) == fused
        m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
        m.prepare_critic_fakes()
        ref = A.new_state(0.5)
        for d in ds:
            m.feed_host("d", **d)
            m.d_step(iteration=0)
            m.ctx.sync()
            st = m.ada_state.cpu().numpy()
            if fused:
                ref = A.update(ref, m.ctx.download(m.ada_logits)[:B], d["labels"], 0.6, images, N_CRITIC)
                assert np.array_equal(st.view(np.int32), ref.view(np.int32)), (st, ref)
        rep = m.ada_report()
        assert rep["updates"] == 1 and rep["p"] in (0.5 - N_CRITIC * B / images, 0.5, 0.5 + N_CRITIC * B / images), rep
        assert abs(rep["r_last"] * N_CRITIC * B - round(rep["r_last"] * N_CRITIC * B)) < 1e-4 and -1 <= rep["r_last"] <= 1, rep
        assert (st[1:4] == 0).all()
        m.feed_host("g", **g)
        m.g_step(iteration=0)
        d_loss, g_loss = m.losses()
        assert np.isfinite(d_loss) and np.isfinite(g_loss)
        gg = m.get_grads(m.PG)
        for k, gk in gg.items():
            assert np.isfinite(gk).all(), k
        assert float(np.abs(gg["Generator/G.Output/Filters"]).max()) > 0
        assert m.ada_report() == rep
    finally:
        m.ctx.close()


def test_unfused_head_reads_the_same_scores_as_the_fused_one(monkeypatch):
    """fp32, one critic step from the same weights and draws: the controller's sums are the same on the fused and the op-by-op route
    (the scores differ in rounding only, and none of this seed's lies at zero)."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B = 8
    rs = np.random.RandomState(12)
    for alg in ("rcgan", "unbiased", "rcgan-u"):
        _, raw = _batch(rs, B)
        dd, _ = _host_draws_ada(rs, B)
        got = []
        for fused in ("1", "0"):
            monkeypatch.setenv("RCGAN_FUSED_HEAD", fused)
            m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="f32", seed=1, use_graphs=False, device_rng=False,
                           arena_bytes=2 << 30, diffaugment=FULL, ada_target=0.6, ada_images=128.0, ada_interval=3, ada_p_init=0.5)
            try:
                m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
                m.d_step(iteration=0)
                m.ctx.sync()
                got.append(m.ada_state.cpu().numpy().copy())
                if fused == "1":
                    lg = m.ctx.download(m.ada_logits)[:B]
                    assert np.abs(A.scores(lg, raw["labels"])).min() > 1e-4, "a real score of this seed sits at zero: pick another"
            finally:
                m.ctx.close()
        assert np.array_equal(got[0], got[1]) and got[0][2] == B and got[0][3] == 1, (alg, got)


def test_state_dict_round_trip_carries_the_controller():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    B, alg = 8, "rcgan"
    rs = np.random.RandomState(77)
    its = []
    for _ in range(3):
        steps = []
        for _ in range(N_CRITIC):
            _, raw = _batch(rs, B)
            dd, gd = _host_draws_ada(rs, B)
            steps.append((raw, dd))
        its.append((steps, gd, dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))))
    kw = dict(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=False, arena_bytes=2 << 30,
              diffaugment=FULL, ada_target=0.1, ada_images=256.0, ada_interval=2, ada_p_init=0.25)

    def iterate(m, it):
        steps, gd, gb = its[it]
        for raw, dd in steps:
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
            m.d_step(iteration=it)
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=it)
        m.iteration = it + 1

    m = CifarRCGAN(**kw)
    try:
        iterate(m, 0)
        iterate(m, 1)
        sd = m.state_dict()
        assert sd["_ada_state"].dtype == np.float32 and sd["_ada_state"].shape == (8,)
        assert sd["_ada_state"][5] == N_CRITIC and sd["_ada_state"][3] == 0, sd["_ada_state"]     # ten steps, five updates
        iterate(m, 2)
        want_p, want_s, want_ada = m.get_params(), m.get_state(), m.ada_state.cpu().numpy().copy()
    finally:
        m.ctx.close()
    m2 = CifarRCGAN(**dict(kw, seed=9, ada_p_init=0.0))
    try:
        m2.load_state_dict(sd)
        m2.ctx.sync()
        assert np.array_equal(m2.ada_state.cpu().numpy(), sd["_ada_state"])
        assert m2.ada_report()["p"] == float(sd["_ada_state"][0])
        iterate(m2, 2)
        got_p, got_s = m2.get_params(), m2.get_state()
        assert np.array_equal(m2.ada_state.cpu().numpy().view(np.int32), want_ada.view(np.int32)), (m2.ada_state.cpu().numpy(), want_ada)
        for k in want_p:
            assert np.array_equal(got_p[k], want_p[k]), k
        for k in want_s:
            assert np.array_equal(got_s[k], want_s[k]), k
        # a checkpoint without the controller (written with the option off) loads: the state stays what the constructor gave
        sd2 = {k: v for k, v in sd.items() if k != "_ada_state"}
        before = m2.ada_state.cpu().numpy().copy()
        m2.load_state_dict(sd2)
        assert np.array_equal(m2.ada_state.cpu().numpy(), before)
    finally:
        m2.ctx.close()


class CountingLib:
    """ctx.lib with a count of the calls of every entry point (one call enqueues the launches of one op)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rcgan_"):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _count_step_calls(**kw):
    """-> (engine facts, calls of one critic step, calls of one generator step) with host-fed inputs of zeros."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=8, dtype="bf16", seed=2, use_graphs=False, device_rng=True,
                   arena_bytes=2 << 30, **kw)
    try:
        facts = dict(ada_state=m.ada_state, ada_logits=m.ada_logits, inp=sorted(k for k in m.inp if k.startswith("aug_")),
                     feed={k: [f[0] for f in v] for k, v in m.feed_layout.items()}, words={k: int(v.numel()) for k, v in m.feed.items()})
        m.d_step(iteration=0)          # warm-up: one-time launches (LDS attributes, self test) stay out of the count
        m.g_step(iteration=0)
        m.ctx.sync()
        lib = m.ctx.lib
        m.ctx.lib = CountingLib(lib)
        try:
            m.d_step(iteration=1)
            d = dict(m.ctx.lib.calls)
            m.ctx.lib.calls.clear()
            m.g_step(iteration=1)
            g = dict(m.ctx.lib.calls)
        finally:
            m.ctx.lib = lib
        m.ctx.sync()
        return facts, d, g
    finally:
        m.ctx.close()


def test_option_off_and_plain_diffaugment_are_the_engines_they_were():
    B, K = 8, 10
    d_fields = ["images", "labels", "labels_random", "labels_biased", "inv_weights", "labels_all"]
    d_words = B * 3072 + 3 * B + B * K + 2 * B
    off, d_off, g_off = _count_step_calls()
    off0, d_off0, g_off0 = _count_step_calls(ada_target=0.0, ada_images=1000, ada_interval=7, ada_p_init=1.0)
    plain, d_plain, g_plain = _count_step_calls(diffaugment=FULL)
    ada, d_ada, g_ada = _count_step_calls(diffaugment=FULL, ada_target=0.6)
    for facts in (off, off0, plain):
        assert facts["ada_state"] is None and facts["ada_logits"] is None
        assert not [k for k in facts["inp"] if "gate" in k]
        assert facts["feed"] == {"d": d_fields, "g": ["labels_random_G", "labels_biased_G"], "gf": ["labels_random_all"]}
        assert facts["words"] == {"d": d_words, "g": 4 * B, "gf": 5 * B, "d5": 5 * d_words}
    assert off["inp"] == off0["inp"] == [] and plain["inp"] == ["aug_u", "aug_u_G"]
    assert ada["inp"] == ["aug_gate", "aug_gate_G", "aug_u", "aug_u_G"] and ada["feed"] == plain["feed"] and ada["words"] == plain["words"]
    # none of the new entry points is called without the option, and the ignored ada_* arguments change nothing
    for calls in (d_off, g_off, d_plain, g_plain):
        assert not [n for n in NEW if n in calls], calls
    assert d_off == d_off0 and g_off == g_off0
    assert d_plain["rcgan_diffaugment_fwd"] == 1 and g_plain["rcgan_diffaugment_fwd"] == 1 and g_plain["rcgan_diffaugment_bwd"] == 1
    # the adaptive probability over plain diffaugment: ONE more call per critic step (the update), none per generator step, and no
    # draw of its own
    swap = lambda c: {{"rcgan_diffaugment_gated_fwd": "rcgan_diffaugment_fwd", "rcgan_diffaugment_sampled_bwd": "rcgan_diffaugment_bwd"}.get(k, k): v
                      for k, v in c.items()}
    assert d_ada["rcgan_rng_fill"] == d_plain["rcgan_rng_fill"] and g_ada["rcgan_rng_fill"] == g_plain["rcgan_rng_fill"]
    assert swap(g_ada) == g_plain
    want = dict(d_plain, rcgan_ada_update=1)
    assert swap(d_ada) == want, (d_ada, d_plain)
