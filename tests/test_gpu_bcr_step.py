"""CifarRCGAN(bcr_real=, bcr_fake=, bcr_policy=): whole critic steps with balanced consistency regularisation.

The reference is built here: oracle.torch_port.CifarTorch's generator, discriminator and projection, unmodified, in float64; the
discriminator evaluated ONCE on the 4B rows [real ; fake ; T(real) ; T(fake)], T = tests/diffaugment_ref.py on the host-fed bcr_u; the
hinge terms on rows [0, 2B) as the oracle's disc_cost forms them, plus lam_real * mean_{i<B} c_i + lam_fake * mean_{B<=i<2B} c_i with
c_i the squared difference of the scores of rows i and i + 2B at row i's label or weight row; differentiated with autograd.

Bounds: those of tests/test_gpu_cifar_step.py (_check / cmp_all there), restated in _compare below.  B = 4 for every algorithm and
precision that file runs, B = 64 for the production precision.  device_rng=False: bcr_u is a step input.
"""
import collections

import numpy as np
import pytest
import torch

from oracle import cifar as oc
from tests import diffaugment_ref as R
from tests.gpu_util import rel_err
from tests.test_gpu_diffaugment_step import FULL, _batch, _host_draws, _iterations, _jittered_variables, _labels_all

pytestmark = pytest.mark.gpu

LAM_R, LAM_F = 10.0, 5.0
POLICY = 7          # POLICY: all three transforms -- on a fresh critic a 4-pixel shift alone moves the scores by ~1e-3


def _u(rs, n):
    return np.minimum(rs.uniform(size=(n, 8)).astype(np.float32), np.float32(R.U_MAX))


def _inputs(alg, B, seed=31):
    rs = np.random.RandomState(seed + B)
    C, raw = _batch(rs, B)
    dd, gd = _host_draws(rs, B)
    dd.pop("aug_u"), gd.pop("aug_u_G")
    dd["bcr_u"] = _u(rs, 2 * B)
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    return C, raw, dd, gd, gb, _jittered_variables(alg)


def bcr_disc_cost(net, cfg, b, bcr_u, lam_r, lam_f, policy):
    """-> (cost, hinge cost, c_real mean, c_fake mean) on the float64 net."""
    alg, B = cfg["algorithm"], len(b["labels"])
    idx = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.long)
    fake = net.generator(b["labels_random"], b["z"])
    real = torch.as_tensor(b["real"], dtype=net.dtype)
    x_all = torch.cat([real, fake], 0)
    x_aug = R.diffaugment(x_all.reshape(-1, 32, 32, 3), bcr_u, policy).reshape(-1, 3072)
    feat, wgan = net.discriminator(torch.cat([x_all, x_aug], 0), True)
    logits = wgan[:, None] + feat @ net.projection(np.arange(10)).t()           # [4B, 10]: every label's logit of every row
    first, second = logits[:2 * B], logits[2 * B:]
    at = lambda lg, lab: lg[torch.arange(len(lab)), idx(lab)]
    if alg == "rcgan-u":
        y = net.C(cfg)[idx(b["labels_random"])]
        hinge = (net.hinge("fake", 1 + first[B:]) * y).sum(1).mean() + net.hinge("real", 1 - at(first[:B], b["labels"])).mean()
        c_real = (at(first[:B], b["labels"]) - at(second[:B], b["labels"])) ** 2
        c_fake = (y * (first[B:] - second[B:]) ** 2).sum(1)
    elif alg == "unbiased":
        w = torch.as_tensor(b["inv_weights"], dtype=net.dtype)
        hinge = (net.hinge("real", 1 - first[:B]) * w).sum(1).mean() + net.hinge("fake", 1 + at(first[B:], b["labels_random"])).mean()
        c_real = (w * (first[:B] - second[:B]) ** 2).sum(1)
        c_fake = (at(first[B:], b["labels_random"]) - at(second[B:], b["labels_random"])) ** 2
    else:
        lab = _labels_all(alg, b)
        d, da = at(first, lab), at(second, lab)
        hinge = net.hinge("real", 1 - d[:B]).mean() + net.hinge("fake", 1 + d[B:]).mean()
        c = (d - da) ** 2
        c_real, c_fake = c[:B], c[B:]
    return hinge + lam_r * c_real.mean() + lam_f * c_fake.mean(), hinge, c_real.mean(), c_fake.mean()


_oracle = {}


def oracle_critic(alg, B, policy=POLICY, lams=(LAM_R, LAM_F)):
    """The float64 reference of one case, computed once and shared."""
    key = (alg, B, policy, lams)
    if key not in _oracle:
        from oracle.torch_port import CifarTorch
        C, raw, dd, gd, gb, variables = _inputs(alg, B)
        P = {n: v.copy() for n, _, v in variables[0] + variables[1] + variables[2]}
        U = {k: v.copy() for k, v in variables[3].items()}
        net = CifarTorch(P, U, torch.float64)
        b = dict(real=oc.preprocess_real(raw["images"], dd["noise"]), z=dd["z"], **raw)
        cost, hinge, cr, cf = bcr_disc_cost(net, dict(algorithm=alg, C=C), b, dd["bcr_u"], lams[0], lams[1], policy)
        names = [k for k in net.P if k.startswith("Discriminator/")]
        grads = dict(zip(names, (g.numpy() for g in torch.autograd.grad(cost, [net.P[k] for k in names]))))
        _oracle[key] = dict(cost=float(cost.detach()), hinge=float(hinge.detach()), real=float(cr.detach()), fake=float(cf.detach()),
                            grads=grads, kink=min(float(t.abs().min()) for t in net.hinge_args.values()))
    return _oracle[key]


def _compare(tag, got, grads, sixteen, B):
    """tests/test_gpu_cifar_step.py's cmp_all, bound for bound."""
    gmax = max(float(np.abs(g).max()) for g in grads.values())
    for k, gref in grads.items():
        a = got[k]
        assert np.isfinite(a).all(), k
        floor = 1e-3 * gmax
        scale = max(float(np.abs(gref).max()), floor)
        err = float(np.abs(a - gref).max()) / scale
        if not sixteen:
            nrm = float(np.linalg.norm(a - gref)) / max(float(np.linalg.norm(gref)), scale)
            print("%s %-60s norm-rel %.3e max err %.3e" % (tag, k, nrm, err))
            assert nrm <= 1e-2 and err <= 1e-1, "%s %s: norm-rel %.3e max err %.3e of scale %.3e" % (tag, k, nrm, err, scale)
        elif np.size(gref) <= 1:
            print("%s %-60s %r want %r" % (tag, k, np.ravel(a)[0], np.ravel(gref)[0]))
            assert abs(float(np.ravel(a)[0]) - float(np.ravel(gref)[0])) <= 1.5 / B, k
        elif float(np.abs(gref).max()) > floor:
            e = rel_err(a, gref)
            cos = float((a.astype(np.float64) * gref).sum() / (np.linalg.norm(a) * np.linalg.norm(gref) + 1e-30))
            print("%s %-60s norm-rel %.3e cos %.4f" % (tag, k, e, cos))
            assert e <= 8e-2 and cos >= 0.95, "%s %s: norm-rel %.3e cos %.4f" % (tag, k, e, cos)
        else:
            assert err <= 0.5, "%s %s: %.3e" % (tag, k, err)


def _engine(alg, B, dtype, variables=None, **kw):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    kw.setdefault("use_graphs", False)
    kw.setdefault("device_rng", False)
    kw.setdefault("arena_bytes", (2 << 30) if B <= 8 else None)
    return CifarRCGAN(algorithm=alg, alpha=0.6, batch_size=B, dtype=dtype, variables=variables, **kw)


CASES = [("rcgan", 4, "f32"), ("rcgan-u", 4, "f32"), ("biased", 4, "f32"), ("unbiased", 4, "f32"),
         ("rcgan", 4, "bf16"), ("rcgan-u", 4, "bf16"), ("rcgan", 4, "f16"), ("rcgan", 64, "bf16")]


@pytest.mark.parametrize("alg,B,dtype", CASES)
def test_critic_step_against_float64(alg, B, dtype):
    C, raw, dd, gd, gb, variables = _inputs(alg, B)
    want = oracle_critic(alg, B)
    print("%s B %d: hinge arguments: nearest to the kink %.3e; cost %r = hinge %r + %g * %r + %g * %r"
          % (alg, B, want["kink"], want["cost"], want["hinge"], LAM_R, want["real"], LAM_F, want["fake"]))
    m = _engine(alg, B, dtype, variables, bcr_real=LAM_R, bcr_fake=LAM_F, bcr_policy=FULL)
    try:
        assert m.bcr and m.bcr_policy == POLICY and m.inp["bcr_u"].shape == (2 * B, 8)
        assert [f[0] for f in m.feed_layout["d"]][-1] == "bcr_u" and "_bcr" not in "".join(m.state_dict())
        assert m.bcr_report() == dict(real=0.0, fake=0.0)
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        d_loss, _ = m.losses()
        rep = m.bcr_report()
        sixteen = dtype != "f32"
        tol = 5e-3 if sixteen else 2e-5
        print("%s B %d %s: loss %r want %r; report %r want %r %r" % (alg, B, dtype, d_loss, want["cost"], rep, want["real"], want["fake"]))
        assert abs(d_loss - want["cost"]) <= tol * max(1.0, abs(want["cost"])), (d_loss, want["cost"])
        _compare("D", m.get_grads(m.PD), want["grads"], sixteen, B)
        # the reported means are the two unweighted terms: the loss bound shared out by the weights
        assert abs(rep["real"] - want["real"]) <= tol * max(1.0, abs(want["cost"])) / LAM_R, (rep, want["real"])
        assert abs(rep["fake"] - want["fake"]) <= tol * max(1.0, abs(want["cost"])) / LAM_F, (rep, want["fake"])
        assert want["real"] > 0 and want["fake"] > 0
    finally:
        m.ctx.close()


def test_one_weight_zero_leaves_that_part_out():
    """bcr_real = 0: no launch for the real part -- its reported mean stays 0, its second-half rows get a zero gradient -- so the cost
    and every critic gradient are those of the float64 reference at lam_real = 0 (fp32 bounds)."""
    alg, B = "rcgan", 4
    C, raw, dd, gd, gb, variables = _inputs(alg, B)
    want = oracle_critic(alg, B, lams=(0.0, LAM_F))
    m = _engine(alg, B, "f32", variables, bcr_real=0.0, bcr_fake=LAM_F, bcr_policy=FULL)
    try:
        m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **dd)
        m.d_step(iteration=0)
        cost = want["hinge"] + LAM_F * want["fake"]
        d_loss, rep = m.losses()[0], m.bcr_report()
        assert abs(d_loss - cost) <= 2e-5 * max(1.0, abs(cost)), (d_loss, cost)
        assert rep["real"] == 0.0 and abs(rep["fake"] - want["fake"]) <= 2e-5 / LAM_F, rep
        assert abs(cost - want["cost"]) <= 1e-12
        _compare("D", m.get_grads(m.PD), want["grads"], False, B)
    finally:
        m.ctx.close()


@pytest.mark.parametrize("alg,B,dtype", [("rcgan", 4, "f32"), ("rcgan-u", 4, "bf16"), ("unbiased", 4, "bf16"), ("rcgan", 64, "bf16")])
def test_the_identity_transform_reports_exactly_zero(alg, B, dtype):
    """Translation only with u3 = u4 = 0.5 is a shift by (0, 0): rows i and i + 2B are the same image, their scores the same bits.  A
    term that is exactly zero adds nothing: loss and critic gradients are the plain engine's (the option off, on its own head route)
    up to rounding -- the bounds of _compare with the plain engine as the reference."""
    C, raw, dd, gd, gb, variables = _inputs(alg, B)
    dd["bcr_u"][:, 3:5] = 0.5
    outs = []
    for lam in (LAM_R, 0.0):
        m = _engine(alg, B, dtype, variables, bcr_real=lam, bcr_fake=lam, bcr_policy="translation")
        try:
            d = dict(dd)
            if not lam:
                d.pop("bcr_u")
                assert "bcr_u" not in m.inp
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **d)
            m.d_step(iteration=0)
            if lam:
                assert m.bcr_report() == dict(real=0.0, fake=0.0)
            outs.append((m.losses()[0], m.get_grads(m.PD)))
        finally:
            m.ctx.close()
    (la, ga), (lb, gb_) = outs
    assert abs(la - lb) <= (5e-3 if dtype != "f32" else 2e-5) * max(1.0, abs(lb)), (la, lb)
    _compare("D", ga, {k: v.astype(np.float64) for k, v in gb_.items()}, dtype != "f32", B)


def _controllers(m):
    out = {}
    if m.ada_state is not None:
        out["ada"] = m.ada_state.cpu().numpy().copy()
    if m.lecam_state is not None:
        out["lecam"] = m.lecam_state.cpu().numpy().copy()
    return out


LECAM_PRESET = np.array([-0.35, 0.45, 1, 0, 0, 0, 0, 0], np.float32)          # {a_R, a_F, updates = 1, ...}: the gate is open


@pytest.mark.parametrize("name,kw", [("diffaugment", dict(diffaugment=FULL)),
                                     ("ada", dict(diffaugment=FULL, ada_target=0.6, ada_images=1000, ada_interval=1, ada_p_init=0.5)),
                                     ("lecam", dict(lecam=0.3, lecam_decay=0.9)),
                                     ("diversity", dict(diversity=0.5))])
def test_coexistence_and_the_controllers_read_the_first_half_only(name, kw, monkeypatch):
    """One critic step and one generator step with each of the other options beside the term, bf16, B = 8, draws on the device.  The
    controllers' states after the critic step equal those of the same step with the option off, bit for bit: they read rows [0, 2B),
    which the term's second half does not move (the op-by-op head on both sides)."""
    monkeypatch.setenv("RCGAN_FUSED_HEAD", "0")
    B, alg = 8, "rcgan"
    rs = np.random.RandomState(5)
    raw = _batch(rs, B)[1]
    gb = dict(labels_random_G=rs.randint(10, size=2 * B), labels_biased_G=rs.randint(10, size=2 * B))
    outs = []
    for on in (True, False):
        bcr = dict(bcr_real=LAM_R, bcr_fake=LAM_F, bcr_policy="translation,cutout") if on else {}
        m = _engine(alg, B, "bf16", None, seed=3, device_rng=True, **kw, **bcr)
        try:
            assert not m.fused_head
            if m.lecam_state is not None:
                with torch.cuda.stream(m.ctx.stream):
                    m.lecam_state.copy_(torch.from_numpy(LECAM_PRESET))
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw)
            m.d_step(iteration=0)
            m.ctx.sync()
            st, d_loss, rep = _controllers(m), m.losses()[0], m.bcr_report()
            m.set_inputs(**gb)
            m.g_step(iteration=0)
            outs.append((st, d_loss, rep))
            assert np.isfinite(d_loss) and np.isfinite(m.losses()[1])
            for grp in (m.PD, m.PG):
                for k, g in m.get_grads(grp).items():
                    assert np.isfinite(g).all(), k
        finally:
            m.ctx.close()
    (sa, la, ra), (sb, lb, rb) = outs
    print(name, "controllers", sa, "loss with the term", la, "without", lb, "report", ra)
    assert rb == dict(real=None, fake=None) and ra["real"] > 0 and ra["fake"] > 0 and la > lb
    assert sorted(sa) == sorted(sb) == {"ada": ["ada"], "lecam": ["lecam"]}.get(name, [])
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), (k, sa[k], sb[k])
    if name == "lecam":
        assert sa["lecam"][2] == 2 and sa["lecam"][0] != LECAM_PRESET[0]


def test_replayed_iteration_equals_launch_by_launch(monkeypatch):
    """Two iterations (five critic steps, a generator step) with the draws on the device: captured graphs -- the five critic steps as
    one -- against the same launches issued one by one: weights, Adam slots, losses and the reported means bit for bit."""
    from rcgan_amd.cifar import N_CRITIC
    B = 8
    its = _iterations(np.random.RandomState(23), B, 2)
    outs = []
    for graphs in (True, False):
        m = _engine("rcgan", B, "bf16", None, seed=5, use_graphs=graphs, device_rng=True, bcr_real=LAM_R, bcr_fake=LAM_F)
        try:
            for it, (ds, g) in enumerate(its):
                m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
                m.prepare_critic_fakes()
                m.critic_steps(ds, iteration=it)
                m.ctx.sync()
                rep = m.bcr_report()
                m.feed_host("g", **g)
                m.g_step(iteration=it)
            m.ctx.sync()
            assert ("d5" in m._graphs) == graphs
            outs.append((m.get_params(), m.PD.m.cpu().numpy().copy(), m.PD.v.cpu().numpy().copy(), m.losses(), rep,
                         m.bcr_rng_state.cpu().numpy().copy()))
        finally:
            m.ctx.close()
    (pa, ma, va, la, ra, sa), (pb, mb, vb, lb, rb, sb) = outs
    print("losses", la, "report", ra, "stream", sa)
    assert la == lb and ra == rb and ra["real"] > 0 and ra["fake"] > 0
    assert np.array_equal(sa, sb) and sa.any(), "the term's random stream did not move by the same draws"
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


class LoggingLib:
    """ctx.lib with the ordered log of the entry points called."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rcgan_"):
            return fn

        def logged(*a):
            self.log.append(name)
            return fn(*a)
        return logged


def _iteration_log(**kw):
    """-> (engine facts, the entry-point log of the critic steps of one full iteration, that of its generator step)."""
    B = 8
    its = _iterations(np.random.RandomState(29), B, 2)
    m = _engine("rcgan", B, "bf16", None, seed=2, device_rng=True, arena_bytes=None, **kw)          # (the arena the engine sizes for itself)
    try:
        facts = dict(inp=sorted(m.inp), feed={k: [f[0] for f in v] for k, v in m.feed_layout.items()},
                     words={k: int(v.numel()) for k, v in m.feed.items()}, state=sorted(m.state_dict()),
                     bcr=(m.bcr, m.x_all4, m.bcr_rng_state, m.bcr_terms), arena=m.ctx.arena.cap)
        logs = []
        for it, (ds, g) in enumerate(its):          # iteration 0: warm-up, one-time launches stay out of the log
            lib = m.ctx.lib
            m.ctx.lib = LoggingLib(lib)
            try:
                m.feed_host("gf", labels_random_all=np.concatenate([d["labels_random"] for d in ds]))
                m.prepare_critic_fakes()
                m.critic_steps(ds, iteration=it)
                d_log = list(m.ctx.lib.log)
                del m.ctx.lib.log[:]
                m.feed_host("g", **g)
                m.g_step(iteration=it)
                logs = (d_log, list(m.ctx.lib.log))
            finally:
                m.ctx.lib = lib
        m.ctx.sync()
        return facts, logs[0], logs[1]
    finally:
        m.ctx.close()


def test_off_is_off_and_the_generator_step_is_unchanged():
    off, d_off, g_off = _iteration_log()
    off0, d_off0, g_off0 = _iteration_log(bcr_real=0.0, bcr_fake=0.0, bcr_policy="translation,cutout")
    on, d_on, g_on = _iteration_log(bcr_real=LAM_R, bcr_fake=LAM_F)
    # off: no buffer, no input, no draw, nothing checkpointed, and every call of the iteration in the same place
    assert off == off0 and off["bcr"] == (False, None, None, None) and "bcr_u" not in off["inp"]
    assert d_off == d_off0 and g_off == g_off0
    assert not [n for n in d_off + g_off + g_on if "consistency" in n]
    # on: the generator step's log is unchanged; nothing is checkpointed; the critic steps take the op-by-op head
    assert g_on == g_off and on["state"] == off["state"] and "bcr_u" in on["inp"] and on["arena"] > off["arena"]
    c_on, c_off = collections.Counter(d_on), collections.Counter(d_off)
    from rcgan_amd.cifar import N_CRITIC
    assert c_on["rcgan_pair_consistency_fwd_bwd"] == 2 * N_CRITIC and c_on["rcgan_proj_head_fwd_bwd"] == 0
    assert c_off["rcgan_proj_head_fwd_bwd"] == N_CRITIC and c_on["rcgan_loss_fwd_bwd"] == 2 * N_CRITIC
    assert c_on["rcgan_diffaugment_fwd"] == N_CRITIC and c_on["rcgan_rng_fill"] == c_off["rcgan_rng_fill"] + N_CRITIC


def test_eval_d_cost_stays_the_plain_dev_cost():
    B, alg = 4, "rcgan"
    C, raw, dd, gd, gb, variables = _inputs(alg, B)
    costs = []
    for lam in (LAM_R, 0.0):
        m = _engine(alg, B, "bf16", variables, bcr_real=lam, bcr_fake=lam)
        try:
            d = dict(dd)
            if not lam:
                d.pop("bcr_u")
            m.set_inputs(labels_all=_labels_all(alg, raw), **raw, **d)
            lib = m.ctx.lib
            m.ctx.lib = LoggingLib(lib)
            try:
                costs.append(m.eval_d_cost())
                log = list(m.ctx.lib.log)
            finally:
                m.ctx.lib = lib
            assert "rcgan_pair_consistency_fwd_bwd" not in log and "rcgan_diffaugment_fwd" not in log
        finally:
            m.ctx.close()
    assert costs[0] == costs[1] and np.isfinite(costs[0]), costs
