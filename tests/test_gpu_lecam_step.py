"""CifarRCGAN(lecam=..., lecam_decay=...): whole steps with the LeCam regulariser.  B = 8, fp32 unless said otherwise.

(a) rcgan, anchors preset to non-trivial values with updates = 1: one critic step against float64 autograd of a subclass of
    oracle.torch_port.CifarTorch that keeps the live hinge arguments and adds lambda R to disc_cost -- bounds those of
    test_gpu_diffaugment_step.test_critic_and_generator_step_against_float64 (2e-5 on the loss, 2e-3 norm-relative per gradient tensor);
    the generator step that follows matches the unregularised oracle and leaves the state alone;
(b) the other three algorithms and the op-by-op head, the same check; one case with DiffAugment + ADA on;
(c) the five critic steps as one captured graph against five d_step() calls: weights, Adam slots and _lecam_state bit for bit, and the
    state after every single step is the reference applied to the logits that step left;
(d) the checkpoint round trip; (e) eval_d_cost is the plain dev cost and leaves the state alone; (f) the option off is the engine it
    was, call by call; (g) bf16 and f16.

The seeds of (a) and (b) were chosen on the CPU (oracle_critic below needs no GPU) so that every hinge argument is further than 1e-3
from its kink; the tests assert it.  (A freshly initialised critic's logits are small: every hinge is active there, about 0.7 from
its kink at each of the seeds 1 .. 12 and 31.  The inactive side is tests/test_gpu_lecam_ops.py's.)
"""
import numpy as np
import pytest
import torch

from oracle import cifar as oc
from tests import lecam_ref as LR
from tests.test_gpu_ada_step import CountingLib, _ada_torch, _host_draws_ada
from tests.test_gpu_diffaugment_step import FULL, _batch, _compare, _host_draws, _iterations, _jittered_variables, _labels_all

pytestmark = pytest.mark.gpu

LAM, DECAY = 0.3, 0.9
PRESET = np.array([-0.35, 0.45, 1, 0, 0, 0, 0, 0], np.float32)          # {a_R, a_F, updates = 1, ...}
ULP = 2.0 ** -23
# algorithm -> seed (chosen on the CPU: see the module docstring); "ada": rcgan under DiffAugment + ADA at p = 0.5
SEEDS = {"rcgan": 31, "biased": 31, "rcgan-u": 31, "unbiased": 31, "ada": 31}


def _lecam_torch(base):
    class LecamTorch(base):
        """The oracle with the live hinge arguments kept and lambda R added to disc_cost: D(real) = 1 - t, D(fake) = t - 1."""
        lam, a_R, a_F = LAM, float(PRESET[0]), float(PRESET[1])

        def hinge(self, name, t):
            self.live[name] = t
            return super().hinge(name, t)

        def disc_cost(self, cfg, b):
            self.live = {}
            cost = super().disc_cost(cfg, b)
            alg, lv = cfg["algorithm"], self.live
            fake = ((lv["fake"] - 1 - self.a_R) ** 2)
            if alg == "rcgan-u":
                y = self.C(cfg)[torch.as_tensor(b["labels_random"], dtype=torch.long)]
                R = (fake * y).sum(1).mean() + ((1 - lv["real"] - self.a_F) ** 2).mean()
            elif alg == "unbiased":
                cols = torch.cat([((1 - lv["real%d" % j] - self.a_F) ** 2).reshape(-1, 1) for j in range(10)], 1)
                R = (cols * torch.as_tensor(b["inv_weights"], dtype=self.dtype)).sum(1).mean() + fake.mean()
            else:
                R = ((1 - lv["real"] - self.a_F) ** 2).mean() + fake.mean()
            self.R = R
            return cost + self.lam * R
    return LecamTorch


def oracle_inputs(key, B=8):
    alg = "rcgan" if key == "ada" else key
    rs = np.random.RandomState(SEEDS[key])
    C, raw = _batch(rs, B)
    dd, gd = _host_draws_ada(rs, B) if key == "ada" else _host_draws(rs, B)
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    if key != "ada":
        dd.pop("aug_u"), gd.pop("aug_u_G")
    return alg, C, raw, dd, gd, gb, _jittered_variables(alg)


_oracle = {}


def oracle_critic(key):
    """-> dict(cost, R, grads, kink, active) of the regularised critic cost in float64, computed once per case and shared."""
    if key not in _oracle:
        from oracle.torch_port import CifarTorch
        alg, C, raw, dd, gd, gb, variables = oracle_inputs(key)
        P = {n: v.copy() for n, _, v in variables[0] + variables[1] + variables[2]}
        U = {k: v.copy() for k, v in variables[3].items()}
        net = _lecam_torch(_ada_torch() if key == "ada" else CifarTorch)(P, U, torch.float64)
        if key == "ada":
            net.aug_u, net.aug_gate, net.p = dd["aug_u"], dd["aug_gate"], 0.5
        cost = net.disc_cost(dict(algorithm=alg, C=C), dict(real=oc.preprocess_real(raw["images"], dd["noise"]), z=dd["z"], **raw))
        names = [k for k in net.P if k.startswith("Discriminator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        _oracle[key] = dict(cost=float(cost.detach()), R=float(net.R.detach()), grads=grads,
                            kink=min(float(t.abs().min()) for t in net.hinge_args.values()),
                            active=sum(int((t > 0).sum()) for t in net.hinge_args.values()),
                            terms=sum(int(t.numel()) for t in net.hinge_args.values()))
    return _oracle[key]


def _parts(alg, d):
    """(labels, wts) of the real and of the fake rows, as the loss terms of the algorithm have them (host arrays)."""
    if alg == "rcgan-u":
        return (d["labels"], None), (None, "confusion")
    if alg == "unbiased":
        return (None, d["inv_weights"]), (d["labels_random"], None)
    la = _labels_all(alg, d)
    return (la[:len(la) // 2], None), (la[len(la) // 2:], None)


def _check_update(m, before, after, d, what=""):
    """after = rcgan_lecam_update(before) on the logits the step's head left in the shared buffer: means within their bounds, anchors
    within decay * 0 + (1 - decay) * (the mean's bound) + 4 ulp (before is the device's own state: no error carried in), counters exact."""
    B = m.B
    part_a, part_b = _parts(m.alg, d)
    if part_b[1] is not None and isinstance(part_b[1], str):
        part_b = (None, m.confusion_matrix_value()[np.asarray(d["labels_random"])].astype(np.float32))
    lg = m.ctx.download(m.ada_logits)
    d32 = float(np.float32(m.lecam_decay))
    ref, (ba, bb) = LR.update_from_logits(before.astype(np.float64), lg, B, d32, part_a, part_b)
    got = after.astype(np.float64)
    assert got[LR.UPDATES] == before[LR.UPDATES] + 1 and got[LR.SKIPPED] == before[LR.SKIPPED] and got[6] == 0 and got[7] == 0, (what, got, ref)
    assert abs(got[LR.MEAN_REAL] - ref[LR.MEAN_REAL]) <= ba and abs(got[LR.MEAN_FAKE] - ref[LR.MEAN_FAKE]) <= bb, (what, got, ref, ba, bb)
    if before[LR.UPDATES] == 0:
        bound = np.array([ba, bb])
    else:
        means = np.array([ref[LR.MEAN_REAL], ref[LR.MEAN_FAKE]])
        bound = (1 - d32) * np.array([ba, bb]) + 4 * ULP * (np.abs(d32 * before[:2].astype(np.float64)) + np.abs((1 - d32) * means))
    assert (np.abs(got[:2] - ref[:2]) <= bound).all(), (what, got, ref, bound)
    return ref


def _preset(m, state=PRESET):
    with torch.cuda.stream(m.ctx.stream):
        m.lecam_state.copy_(torch.from_numpy(np.asarray(state, np.float32)))
    m.ctx.sync()


def _critic_step_against_float64(key, monkeypatch, fused=True, generator_too=False):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    monkeypatch.setenv("RCGAN_FUSED_HEAD", "1" if fused else "0")
    alg, C, raw, dd, gd, gb, variables = oracle_inputs(key)
    want = oracle_critic(key)
    print("%s: hinge arguments: nearest to the kink %.3e, %d of %d active" % (key, want["kink"], want["active"], want["terms"]))
    assert want["kink"] > 1e-3 and want["active"] > 0, "a hinge term sits at its kink (or none is active) at this seed: pick another"
    kw = dict(diffaugment=FULL, ada_target=0.6, ada_images=1e12, ada_interval=1, ada_p_init=0.5) if key == "ada" else {}
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=8, dtype="f32", use_graphs=False, device_rng=False, variables=variables,
                   arena_bytes=2 << 30, lecam=LAM, lecam_decay=DECAY, **kw)
    try:
        assert m.fused_head == fused and (m.ada_logits is not None) == fused and m.lecam_state is not None
        assert m.lecam_report() == dict(a_real=0.0, a_fake=0.0, mean_real=0.0, mean_fake=0.0, reg=0.0, updates=0, skipped=0)
        _preset(m)
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        d_loss, _ = m.losses()
        print("%s: loss %r want %r; R %r want %r" % (key, d_loss, want["cost"], m.lecam_report()["reg"], want["R"]))
        assert abs(d_loss - want["cost"]) <= 2e-5 * max(1.0, abs(want["cost"])), (d_loss, want["cost"])
        grads = want["grads"]
        _compare("D", m.get_grads(m.PD), grads, 2e-3)
        rep = m.lecam_report()
        assert abs(rep["reg"] - want["R"]) <= 2e-5 * max(1.0, abs(want["R"])), (rep, want["R"])
        assert rep["updates"] == 2 and rep["skipped"] == 0
        after = m.lecam_state.cpu().numpy().copy()
        if fused:
            _check_update(m, PRESET, after, dict(raw, labels_all=_labels_all(alg, raw)), key)
        else:
            # the op-by-op route hands the controller scores that differ from the fused head's in rounding only: the anchors moved
            # from the preset by (1 - decay) of a mean of the size the oracle's logits have
            assert np.isfinite(after).all() and after[0] != PRESET[0] and after[1] != PRESET[1]
        if generator_too:
            from oracle.torch_port import CifarTorch
            P2, U2 = m.get_params(), m.get_state()
            m.set_inputs(**gb, **gd)
            m.g_step(iteration=1)
            net = CifarTorch(P2, U2, torch.float64)
            cost = net.gen_cost(dict(algorithm=alg, C=C), dict(z=gd["z_G"], **gb))
            names = [k for k in net.P if k.startswith("Generator/")]
            ggrads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
            _, g_loss = m.losses()
            assert abs(g_loss - float(cost.detach())) <= 2e-5 * max(1.0, abs(float(cost.detach()))), (g_loss, float(cost.detach()))
            _compare("G", m.get_grads(m.PG), ggrads, 2e-3)
            assert np.array_equal(m.lecam_state.cpu().numpy().view(np.int32), after.view(np.int32)), "the generator step touched the anchors"
    finally:
        m.ctx.close()


def test_critic_and_generator_step_against_float64(monkeypatch):
    _critic_step_against_float64("rcgan", monkeypatch, generator_too=True)


@pytest.mark.parametrize("key,fused", [("biased", True), ("rcgan-u", True), ("unbiased", True), ("rcgan", False), ("rcgan-u", False),
                                       ("unbiased", False), ("ada", True)])
def test_critic_step_on_the_other_routes_against_float64(key, fused, monkeypatch):
    _critic_step_against_float64(key, monkeypatch, fused=fused)


def test_critic_steps_as_one_graph_equal_single_steps(monkeypatch):
    """bf16, draws on the device: the anchors move inside the captured graph, the loss launches of step k + 1 read what step k left."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    B = 8
    its = _iterations(np.random.RandomState(23), B, 2)
    outs = []
    for one_graph in (True, False):
        monkeypatch.setenv("RCGAN_CRITIC_GRAPH", "1" if one_graph else "0")
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=5, use_graphs=True, device_rng=True,
                       arena_bytes=2 << 30, lecam=LAM, lecam_decay=DECAY)
        try:
            states, crit = [], []
            for it, (ds, g) in enumerate(its):
                m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
                m.prepare_critic_fakes()
                assert m._critic_graph_ok() == one_graph
                if one_graph:
                    m.critic_steps(ds, iteration=it * 9000)
                else:
                    for d in ds:
                        before = m.lecam_state.cpu().numpy().copy()
                        m.feed_host("d", **d)
                        m.d_step(iteration=it * 9000)
                        m.ctx.sync()
                        _check_update(m, before, m.lecam_state.cpu().numpy(), d, "iteration %d" % it)
                m.ctx.sync()
                states.append(m.lecam_state.cpu().numpy().copy())
                crit.append(dict({n: m.PD.get(n) for n in m.PD.names}, _m=m.PD.m.cpu().numpy().copy(), _v=m.PD.v.cpu().numpy().copy()))
                m.feed_host("g", **g)
                m.g_step(iteration=it * 9000)
            assert ("d5" in m._graphs) == one_graph
            m.ctx.sync()
            outs.append((states, crit, m.get_params(), m.lecam_report()))
        finally:
            m.ctx.close()
    (sa, ca, pa, ra), (sb, cb, pb, rb) = outs
    print("report", rb)
    assert ra == rb and rb["updates"] == 2 * N_CRITIC and rb["skipped"] == 0 and rb["a_real"] != rb["a_fake"]
    for it in range(2):
        assert np.array_equal(sa[it].view(np.int32), sb[it].view(np.int32)), ("_lecam_state after iteration %d" % it, sa[it], sb[it])
        for k in ca[it]:
            assert np.array_equal(ca[it][k], cb[it][k]), "critic weights / Adam slots after iteration %d: %s" % (it, k)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def _host_iterations(seed, B, n_it, alg="rcgan"):
    from rcgan_amd.cifar import N_CRITIC
    rs = np.random.RandomState(seed)
    its = []
    for _ in range(n_it):
        steps = []
        for _ in range(N_CRITIC):
            _, raw = _batch(rs, B)
            dd, gd = _host_draws(rs, B)
            dd.pop("aug_u"), gd.pop("aug_u_G")
            steps.append((raw, dd))
        its.append((steps, gd, dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))))
    return its


def test_state_dict_round_trip_carries_the_anchors():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import N_CRITIC, CifarRCGAN
    B, alg = 8, "rcgan"
    its = _host_iterations(77, B, 3)
    kw = dict(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=False, arena_bytes=2 << 30,
              lecam=LAM, lecam_decay=DECAY)

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
        assert sd["_lecam_state"].dtype == np.float32 and sd["_lecam_state"].shape == (8,)
        assert sd["_lecam_state"][LR.UPDATES] == 2 * N_CRITIC and sd["_lecam_state"][LR.SKIPPED] == 0, sd["_lecam_state"]
        iterate(m, 2)
        want_p, want_s, want_st = m.get_params(), m.get_state(), m.lecam_state.cpu().numpy().copy()
    finally:
        m.ctx.close()
    m2 = CifarRCGAN(**dict(kw, seed=9))
    try:
        m2.load_state_dict(sd)
        m2.ctx.sync()
        assert np.array_equal(m2.lecam_state.cpu().numpy().view(np.int32), sd["_lecam_state"].view(np.int32))
        assert m2.lecam_report()["a_real"] == float(sd["_lecam_state"][0])
        iterate(m2, 2)
        got_p, got_s = m2.get_params(), m2.get_state()
        assert np.array_equal(m2.lecam_state.cpu().numpy().view(np.int32), want_st.view(np.int32)), (m2.lecam_state.cpu().numpy(), want_st)
        for k in want_p:
            assert np.array_equal(got_p[k], want_p[k]), k
        for k in want_s:
            assert np.array_equal(got_s[k], want_s[k]), k
        # a checkpoint without the anchors (written with the option off) loads: the state stays what it was
        before = m2.lecam_state.cpu().numpy().copy()
        m2.load_state_dict({k: v for k, v in sd.items() if k != "_lecam_state"})
        assert np.array_equal(m2.lecam_state.cpu().numpy(), before)
    finally:
        m2.ctx.close()


def test_eval_d_cost_is_the_plain_cost_and_leaves_the_state_alone():
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B, alg = 8, "rcgan"
    (steps, _, _), = _host_iterations(11, B, 1)
    raw, dd = steps[0]
    costs = []
    for lam in (LAM, 0.0):
        m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=False, arena_bytes=2 << 30,
                       lecam=lam, lecam_decay=DECAY)
        try:
            if lam:
                _preset(m)
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
            lib = m.ctx.lib
            m.ctx.lib = CountingLib(lib)
            try:
                costs.append(m.eval_d_cost())
                calls = dict(m.ctx.lib.calls)
            finally:
                m.ctx.lib = lib
            assert not [n for n in calls if "lecam" in n or "_reg_" in n], calls
            if lam:
                assert np.array_equal(m.lecam_state.cpu().numpy().view(np.int32), PRESET.view(np.int32))
        finally:
            m.ctx.close()
    assert costs[0] == costs[1] and np.isfinite(costs[0]), costs


def _count_calls(**kw):
    """-> (engine facts, calls of one critic step, calls of one generator step), counted as tests/test_gpu_ada_step.py counts them."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=8, dtype="bf16", seed=2, use_graphs=False, device_rng=True,
                   arena_bytes=2 << 30, **kw)
    try:
        facts = dict(lecam_state=m.lecam_state, lecam_R=m.lecam_R, ada_logits=m.ada_logits, state_keys=sorted(k for k in m.state_dict() if k.startswith("_")))
        m.d_step(iteration=0)          # warm-up: one-time launches stay out of the count
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


def test_option_off_is_the_engine_it_was():
    off, d_off, g_off = _count_calls()
    off0, d_off0, g_off0 = _count_calls(lecam=0.0, lecam_decay=0.5)
    on, d_on, g_on = _count_calls(lecam=LAM)
    for facts in (off, off0):
        assert facts["lecam_state"] is None and facts["lecam_R"] is None and facts["ada_logits"] is None
        assert "_lecam_state" not in facts["state_keys"]
    assert off["state_keys"] == off0["state_keys"]
    assert d_off == d_off0 and g_off == g_off0
    for calls in (d_off, g_off, g_on):
        assert not [n for n in calls if "lecam" in n or "_reg_" in n], calls
    # on: the head call is the regularised one, ONE more call per critic step (the update), the generator step unchanged
    assert on["lecam_state"] is not None and on["ada_logits"] is not None and "_lecam_state" in on["state_keys"]
    assert g_on == g_off
    swapped = {{"rcgan_proj_head_reg_fwd_bwd": "rcgan_proj_head_fwd_bwd"}.get(k, k): v for k, v in d_on.items()}
    assert swapped == dict(d_off, rcgan_lecam_update=1), (d_on, d_off)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_sixteen_bit_steps(dtype):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    B, alg = 8, "rcgan"
    (steps, gd, gb), = _host_iterations(5, B, 1)
    m = CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype=dtype, seed=2, use_graphs=False, device_rng=False, arena_bytes=2 << 30,
                   lecam=LAM, lecam_decay=DECAY)
    try:
        for k, (raw, dd) in enumerate(steps[:2]):
            before = m.lecam_state.cpu().numpy().copy()
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
            m.d_step(iteration=0)
            m.ctx.sync()
            _check_update(m, before, m.lecam_state.cpu().numpy(), dict(raw, labels_all=_labels_all(alg, raw)), "%s step %d" % (dtype, k))
            d_loss, _ = m.losses()
            assert np.isfinite(d_loss)
            for name, gk in m.get_grads(m.PD).items():
                assert np.isfinite(gk).all(), name
            rep = m.lecam_report()
            assert (rep["reg"] == 0.0) == (k == 0), rep            # the gate: closed in the first step, open from the second
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=0)
        assert np.isfinite(m.losses()[1])
    finally:
        m.ctx.close()
