"""CifarRCGAN(diversity=..., diversity_tau=...): whole generator steps with the diversity-sensitive term.  B = 8.

(a) fp32: one generator step from the initial (jittered) weights against float64 autograd of a subclass of
    oracle.torch_port.CifarTorch that keeps `fake` and adds the term to gen_cost -- the bounds of
    test_gpu_diffaugment_step.test_critic_and_generator_step_against_float64 (2e-5 on the loss, 2e-3 norm-relative per gradient
    tensor): rcgan with the fused and the op-by-op head, the other three algorithms, the permutation classifier, DiffAugment.
    The cases (seed, weight, clamp) were chosen on the CPU (oracle_step below needs no GPU) so that no pair's ratio is within 1e-3
    of the clamp, the clamp splits the pairs, and the term moves the generator's gradient by far more than the bound: all asserted.
    One more condition decided the seeds, also on the CPU: batch norm over the 16 fakes of a step is badly conditioned at many
    draws, and the SAME oracle evaluated by PyTorch in fp32 is then itself further than the 2e-3 bound from its float64 value
    (3.3e-3 at seed 32 for biased, 3.3e-3 at 34 for unbiased, 2.0e-3 at 35 for perm; worst tensor, norm-relative), which no fp32
    implementation can beat.  The seeds below keep the fp32 oracle within 1e-3 of float64 on every generator tensor (rcgan 31:
    7.6e-4, biased 52: 4.2e-4, rcgan-u 33: 8.1e-4, unbiased 73: 7.5e-4, perm 92: 9.2e-4, aug 36: 6.3e-4).
(b) bf16, fp16 with the static and with the dynamic loss scale against the storage-matched oracle (CifarTorch(storage=...)) with the
    term on the stored fakes and latents, at the 16-bit generator-step bounds of tests/test_gpu_cifar_step.py for B = 8 (2e-2 on the
    loss, 2.5e-1 norm-relative and cosine >= 0.95 per gradient tensor).
(c) the captured generator step equals the eager one bit for bit; (d) the critic steps are unchanged and the option off makes the
    parent's calls one for one; (e) diversity_report() is the reference on the downloaded fakes and latents; (f) unpaired labels are
    masked and their rows keep the critic-only gradient."""
import numpy as np
import pytest
import torch

from tests import diversity_ref as DR
from tests.gpu_util import half_round, rel_err
from tests.test_gpu_ada_step import CountingLib
from tests.test_gpu_diffaugment_step import FULL, _batch, _compare, _host_draws, _iterations

pytestmark = pytest.mark.gpu

B = 8
# key -> (algorithm, fused head, perm, augment, seed, weight, tau); chosen on the CPU: see (a)
CASES = {
    "rcgan": ("rcgan", True, False, False, 31, 2.0, 0.44),
    "rcgan-unfused": ("rcgan", False, False, False, 31, 2.0, 0.44),
    "biased": ("biased", True, False, False, 52, 2.0, 0.448),
    "rcgan-u": ("rcgan-u", True, False, False, 33, 2.0, 0.47),
    "unbiased": ("unbiased", True, False, False, 73, 2.0, float("inf")),
    "perm": ("rcgan", True, True, False, 92, 2.0, 0.45),
    "aug": ("rcgan", True, False, True, 36, 2.0, 0.47),
}


def _variables(alg, perm):
    from rcgan_amd.cifar import create_variables
    gs, ds, cs, U = create_variables(0, alg, perm, "linear", True, 0.2)
    rs = np.random.RandomState(3)

    def jitter(specs):      # de-trivialise the zero-initialised tensors (biases, condBN tables) so their gradients matter
        out = []
        for n, shp, v in specs:
            if n.endswith("/Biases") or n.endswith("/b") or "CondBatchNorm" in n:
                v = (v + 0.1 * rs.randn(*shp)).astype(np.float32)
            out.append((n, shp, v))
        return out
    return jitter(gs), jitter(ds), cs, U


def _div_torch(base):
    class DivTorch(base):
        """The oracle with `fake` kept and the term added to gen_cost, on the unaugmented fakes."""
        lam, tau, z_term = 0.0, float("inf"), None

        def generator(self, labels, z):
            self.fake = super().generator(labels, z)
            return self.fake

        def gen_cost(self, cfg, b):
            cost = super().gen_cost(cfg, b)
            fake, n = self.fake, self.fake.shape[0] // 2
            z = torch.as_tensor(np.asarray(self.z_term if self.z_term is not None else b["z"]), dtype=self.dtype)
            lab = torch.as_tensor(np.asarray(b["labels_random_G"]))
            r = (fake[:n] - fake[n:]).abs().mean(1) / (z[:n] - z[n:]).abs().mean(1)
            m = (lab[:n] == lab[n:]).to(self.dtype)
            self.plain_cost = cost
            return cost - (self.lam / n) * (m * torch.clamp(r, max=self.tau)).sum()
    return DivTorch


def _aug_torch():
    from oracle.torch_port import CifarTorch
    from tests import diffaugment_ref as R

    class AugTorch(CifarTorch):
        aug_u, policy = None, 7

        def discriminator(self, x, update):
            x = R.diffaugment(x.reshape(-1, 32, 32, 3), self.aug_u, self.policy).reshape(-1, 3072)
            return super().discriminator(x, update)
    return AugTorch


def case_inputs(key, paired=True, mode="f32"):
    from rcgan_amd.cifar import pair_generator_labels
    alg, fused, perm, aug, seed, lam, tau = CASES[key]
    rs = np.random.RandomState(seed)
    C, _ = _batch(rs, B)
    _, gd = _host_draws(rs, B)
    if not aug:
        gd.pop("aug_u_G")
    gd["z_G"] = half_round(mode, gd["z_G"])                  # (what the device holds: z_G lives in the activation dtype)
    rnd, bia = rs.randint(10, size=2 * B), rs.randint(10, size=2 * B)
    if paired:
        rnd, bia = pair_generator_labels(rnd, bia, B)
    return alg, C, gd, dict(labels_random_G=rnd, labels_biased_G=bia), _variables(alg, perm)


_oracle = {}


def oracle_step(key, mode="f32", grad_scale=1.0, paired=True):
    """-> dict(cost, plain, grads, plain_grads, ref) of the generator cost with the term: float64, or storage-matched for a 16-bit
    mode.  Needs no GPU; computed once per case and shared."""
    ck = (key, mode, grad_scale, paired)
    if ck not in _oracle:
        from oracle.torch_port import CifarTorch
        alg, fused, perm, aug, seed, lam, tau = CASES[key]
        alg, C, gd, gb, variables = case_inputs(key, paired, mode)
        P = {n: v.copy() for n, _, v in variables[0] + variables[1] + variables[2]}
        U = {k: v.copy() for k, v in variables[3].items()}
        cfg = dict(algorithm=alg, C=C, perm_classifier=perm, perm_multiplier=1.0)
        kw = dict(storage=mode, grad_scale=grad_scale) if mode != "f32" else {}
        net = _div_torch(_aug_torch() if aug else CifarTorch)(P, U, torch.float64, **kw)
        net.lam, net.tau = lam, tau
        if aug:
            net.aug_u = gd["aug_u_G"]
        cost = net.gen_cost(cfg, dict(z=gd["z_G"], **gb))
        names = [k for k in net.P if k.startswith("Generator/") or k == "confusion_logits"]
        take = lambda c, keep: {k: (g.numpy() if g is not None else np.zeros(tuple(net.P[k].shape)))
                                for k, g in zip(names, torch.autograd.grad(c, [net.P[k] for k in names], allow_unused=True, retain_graph=keep))}
        grads, plain_grads = take(cost, True), take(net.plain_cost, False)
        ref = DR.pair_diversity(net.fake.detach().numpy(), gd["z_G"], gb["labels_random_G"], lam, tau)
        _oracle[ck] = dict(cost=float(cost.detach()), plain=float(net.plain_cost.detach()), grads=grads, plain_grads=plain_grads, ref=ref)
    return _oracle[ck]


def _assert_case_is_decisive(key, want):
    """The conditions under which a comparison with the oracle means something: no ratio at the clamp, the clamp splits the pairs (or
    is off), no pair masked, and the term moves the image-end filter gradient by more than fifty times the fp32 bound."""
    alg, fused, perm, aug, seed, lam, tau = CASES[key]
    ref = want["ref"]
    gap = DR.min_relative_gap_to_tau(ref, tau)
    k = "Generator/G.Output/Filters"
    moved = rel_err(want["grads"][k], want["plain_grads"][k])
    print("%s: ratios %s, gap to tau %.3e, clamped %d of %d, term %.6f of cost %.6f, moves %s by %.3e" % (
        key, np.array2string(ref["ratio"], precision=4), gap, ref["clamped"].sum(), B, want["cost"] - want["plain"], want["cost"], k, moved))
    assert gap >= 1e-3, "a ratio sits within 1e-3 of the clamp: pick another seed or clamp"
    assert ref["mask"].all()
    if np.isfinite(tau):
        assert ref["clamped"].any() and not ref["clamped"].all()
    assert moved >= 0.1


class _Keep:
    """Records what cifar.Generator returns in a step (the step's `fake`, alive in the arena until the next step begins)."""

    def __init__(self, monkeypatch):
        from rcgan_amd import cifar
        self.fake, gen = None, cifar.Generator

        def wrapped(*a, **k):
            self.fake = gen(*a, **k)
            return self.fake
        monkeypatch.setattr(cifar, "Generator", wrapped)


def _engine(key, mode, monkeypatch, variables, **kw):
    from rcgan_amd.cifar import CifarRCGAN
    alg, fused, perm, aug, seed, lam, tau = CASES[key]
    monkeypatch.setenv("RCGAN_FUSED_HEAD", "1" if fused else "0")
    args = dict(algorithm=alg, alpha=0.6, batch_size=B, dtype=mode, use_graphs=False, device_rng=False, variables=variables, arena_bytes=2 << 30,
                perm_classifier=perm, perm_multiplier=1.0, confuse_init=True, diffaugment=FULL if aug else "", diversity=lam, diversity_tau=tau)
    args.update(kw)
    m = CifarRCGAN(**args)
    assert m.fused_head == fused
    return m


@pytest.mark.parametrize("key", list(CASES))
def test_generator_step_against_float64(key, monkeypatch):
    import rcgan_amd  # noqa: F401
    alg, C, gd, gb, variables = case_inputs(key)
    want = oracle_step(key)
    _assert_case_is_decisive(key, want)
    keep = _Keep(monkeypatch)
    m = _engine(key, "f32", monkeypatch, variables)
    try:
        assert m.diversity_report() == dict(ratio_mean=0.0, clamped=0.0, masked=0.0)          # (the buffer starts at zero)
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=1)
        _, g_loss = m.losses()
        print("%s: loss %r want %r" % (key, g_loss, want["cost"]))
        assert abs(g_loss - want["cost"]) <= 2e-5 * max(1.0, abs(want["cost"])), (g_loss, want["cost"])
        got = m.get_grads(m.PG)
        if m.PC is not None:
            got.update(m.get_grads(m.PC))
        _compare("G", got, want["grads"], 2e-3)
        # the report is the reference on what the device holds
        fake, z = m.ctx.download(keep.fake), m.ctx.download(m.inp["z_G"])
        mine = DR.pair_diversity(fake, z, gb["labels_random_G"], CASES[key][5], CASES[key][6])
        rep, ref = m.diversity_report(), DR.report(mine["ratio"], CASES[key][6])
        assert rep["masked"] == 0.0 and rep["clamped"] == ref["clamped"], (rep, ref)
        assert abs(rep["ratio_mean"] - ref["ratio_mean"]) <= 1e-6 * ref["ratio_mean"], (rep, ref)
        assert (np.abs(m.ctx.download(m.diversity_ratio) - mine["ratio"]) <= 8 * np.spacing(mine["ratio"].astype(np.float32))).all()
        assert "_diversity" not in " ".join(m.state_dict())                                  # stateless: nothing is checkpointed
    finally:
        m.ctx.close()


def _compare16(tag, got, grads, tol=2.5e-1, cos_min=0.95):
    """The 16-bit rule of tests/test_gpu_cifar_step.py: norm-relative and cosine per tensor; a tensor whose true gradient is zero
    stays under half the floor."""
    gmax = max(float(np.abs(g).max()) for g in grads.values())
    floor, bad = 1e-3 * gmax, []
    for k, gref in grads.items():
        a = got[k].astype(np.float64)
        assert np.isfinite(a).all(), k
        if float(np.abs(gref).max()) > floor:
            e = rel_err(a, gref)
            cos = float((a * gref).sum() / (np.linalg.norm(a) * np.linalg.norm(gref) + 1e-30))
            print("%s %-60s norm-rel %.3e cos %.5f" % (tag, k, e, cos))
            if not (e <= tol and cos >= cos_min):
                bad.append("%s %s: norm-rel %.3e cos %.5f" % (tag, k, e, cos))
        elif float(np.abs(a - gref).max()) / floor > 0.5:
            bad.append("%s %s: %.3e of the floor" % (tag, k, float(np.abs(a - gref).max()) / floor))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode,dynamic", [("bf16", False), ("f16", False), ("f16", True)])
def test_sixteen_bit_generator_step_against_the_storage_matched_oracle(mode, dynamic, monkeypatch):
    import rcgan_amd  # noqa: F401
    key = "rcgan"
    alg, C, gd, gb, variables = case_inputs(key, mode=mode)
    scale = 1024.0 if mode == "f16" else 1.0
    want = oracle_step(key, mode, scale)
    print("%s: ratios %s, gap %.3e" % (mode, want["ref"]["ratio"], DR.min_relative_gap_to_tau(want["ref"], CASES[key][6])))
    assert DR.min_relative_gap_to_tau(want["ref"], CASES[key][6]) >= 1e-3 and want["ref"]["mask"].all()
    m = _engine(key, mode, monkeypatch, variables, dynamic_loss_scale=dynamic)
    try:
        assert m.dynamic_ls == dynamic and (m.loss_scale_state()["scale"] if dynamic else m.loss_scale) == scale
        m.set_inputs(**gb, **gd)
        m.g_step(iteration=1)
        _, g_loss = m.losses()
        print("%s dynamic %d: loss %r want %r" % (mode, dynamic, g_loss, want["cost"]))
        assert abs(g_loss - want["cost"]) <= 2e-2 * max(1.0, abs(want["cost"])), (g_loss, want["cost"])
        _compare16("G " + mode, m.get_grads(m.PG), want["grads"])
        rep = m.diversity_report()
        assert rep["masked"] == 0.0 and np.isfinite(rep["ratio_mean"]) and rep["ratio_mean"] > 0
        if dynamic:
            assert m.loss_scale_state()["skipped_steps"] == 0
    finally:
        m.ctx.close()


def test_captured_generator_step_equals_the_eager_one(monkeypatch):
    """bf16, draws on the device, rcgan with the permutation classifier and DiffAugment on: three generator steps captured (the
    first runs eagerly and is captured, the others are replays) against three steps launch by launch."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN, pair_generator_labels
    its = _iterations(np.random.RandomState(23), B, 3)
    outs = []
    for graphs in (True, False):
        m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=5, use_graphs=graphs, device_rng=True, arena_bytes=2 << 30,
                       perm_classifier=True, diffaugment=FULL, diversity=2.0, diversity_tau=0.46)
        try:
            ratios = []
            for it, (_, g) in enumerate(its):
                rnd, bia = pair_generator_labels(g["labels_random_G"], g["labels_biased_G"], B)
                m.feed_host("g", labels_random_G=rnd, labels_biased_G=bia)
                m.g_step(iteration=it)
                ratios.append((m.ctx.download(m.diversity_ratio).copy(), m.losses()[1], m.diversity_report()))
            assert ("g" in m._graphs) == graphs
            outs.append((ratios, m.get_params()))
        finally:
            m.ctx.close()
    (ra, pa), (rb, pb) = outs
    for it in range(3):
        print("iteration %d: %r" % (it, ra[it][2]))
        assert np.array_equal(ra[it][0].view(np.uint32), rb[it][0].view(np.uint32)) and ra[it][1] == rb[it][1], it
        assert ra[it][2]["masked"] == 0.0 and ra[it][2]["ratio_mean"] > 0
    assert not np.array_equal(ra[0][0], ra[1][0])                                            # (fresh latents on every replay)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def _count_calls(**kw):
    """-> (calls of one critic step, calls of one generator step, weights after them), as tests/test_gpu_lecam_step.py counts."""
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    m = CifarRCGAN(algorithm="rcgan", alpha=0.6, batch_size=B, dtype="bf16", seed=2, use_graphs=False, device_rng=True, arena_bytes=2 << 30, **kw)
    try:
        m.d_step(iteration=0)          # warm-up: one-time launches stay out of the count
        m.g_step(iteration=0)
        m.ctx.sync()
        after_d = {n: m.PD.get(n) for n in m.PD.names}
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
        return d, g, after_d, m.get_params(), m.diversity_ratio, sorted(m.state_dict())
    finally:
        m.ctx.close()


def test_option_off_is_the_engine_it_was_and_the_critic_steps_are_unchanged():
    d_off, g_off, c_off, p_off, buf_off, keys_off = _count_calls()
    d_off0, g_off0, c_off0, p_off0, buf_off0, keys_off0 = _count_calls(diversity=0.0, diversity_tau=0.5)
    d_on, g_on, c_on, p_on, buf_on, keys_on = _count_calls(diversity=1.0, diversity_tau=0.5)
    assert buf_off is None and buf_off0 is None and buf_on is not None
    assert keys_off == keys_off0 == keys_on                                                  # nothing is added to state_dict
    assert d_off == d_off0 == d_on and g_off == g_off0
    for calls in (d_off, g_off, d_on):
        assert not [n for n in calls if "diversity" in n], calls
    assert g_on == dict(g_off, rcgan_pair_diversity_fwd_bwd=1), (g_on, g_off)                # ONE more call per generator step
    for k in p_off:
        assert np.array_equal(p_off[k], p_off0[k]), k
    # the critic step before the first generator step that carries the term: the same bits with the option on
    for k in c_off:
        assert np.array_equal(c_off[k], c_on[k]), k
    assert any(not np.array_equal(p_off[k], p_on[k]) for k in p_off if k.startswith("Generator/"))


def test_unpaired_labels_are_masked_and_keep_the_critic_only_gradient(monkeypatch):
    import rcgan_amd  # noqa: F401
    key = "rcgan"
    alg, C, gd, gb, variables = case_inputs(key, paired=False)
    rnd = gb["labels_random_G"]
    unequal = rnd[:B] != rnd[B:]
    assert unequal.any() and not unequal.all(), "this draw has no pair of either kind"       # (seed 31: asserted, not assumed)
    keep = _Keep(monkeypatch)
    rows = []
    for lam in (CASES[key][5], 0.0):
        m = _engine(key, "f32", monkeypatch, variables, diversity=lam)
        try:
            m.set_inputs(**gb, **gd)
            m.g_step(iteration=1)
            rows.append(m.ctx.download(keep.fake.grad).copy())
            if lam:
                rep = m.diversity_report()
                ratio = m.ctx.download(m.diversity_ratio)
                assert rep["masked"] == unequal.mean() > 0 and np.array_equal(ratio < 0, unequal) and (ratio[unequal] == -1).all(), (rep, ratio)
                want = DR.pair_diversity(m.ctx.download(keep.fake), gd["z_G"], rnd, lam, CASES[key][6])
                assert np.array_equal(want["mask"], ~unequal) and np.isfinite(m.losses()[1])
        finally:
            m.ctx.close()
    on, off = rows
    both = np.concatenate([unequal, unequal])
    assert np.array_equal(on[both].view(np.uint32), off[both].view(np.uint32)), "a masked pair's rows differ from the critic-only gradient"
    assert not np.array_equal(on[~both], off[~both])
