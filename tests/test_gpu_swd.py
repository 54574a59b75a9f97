"""The sliced Wasserstein distance on the GPU (csrc/swd.hip, rcgan_amd/swd.py) against the float64 restatement (tests/swd_ref.py).

The sort is compared bit for bit.  Moments and projections are compared under the bound DERIVED in the header of csrc/swd.hip
(``swd_ref.projection_bound`` restates it; nothing is tuned): with e the largest bound of a set's projections, sorting being
1-Lipschitz in the sup norm, |SWD_gpu - SWD_ref| <= 1e3 (e_a + e_b) per level."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import swd_ref as SR
from tests.gpu_util import make_ctx
from tests.test_swd_cpu import K, PER_CLASS, orderings, templates, world_inputs

pytestmark = pytest.mark.gpu

CHUNK = 8192                                  # SWD_SORT_CHUNK of csrc/swd.hip
N_DIR = 128


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx("f32", arena=1 << 20)
    yield c
    c.close()


def dev(ctx, a):
    with torch.cuda.stream(ctx.stream):
        return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


# ------------------------------------------------------------------------------------------------------------------ the sort
def keys(bits):
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def sorted_bits(rows):
    """np.sort of the rows' bits in the total order of the sign-flip key."""
    k = np.sort(keys(rows.view(np.uint32)), axis=1)
    return k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


@pytest.mark.parametrize("width", [1, 2, 64, CHUNK, 2 * CHUNK, 4 * CHUNK])
def test_rows_come_out_as_the_sort_of_their_bits(ctx, width):
    from rcgan_amd import swd
    rs = np.random.RandomState(width)
    a = rs.randint(-40, 40, size=width).astype(np.float32) / 8                     # duplicates
    special = np.array([0.0, -0.0, np.inf, -np.inf, -0.0, 0.0, np.inf, 1e-45, -1e-45], np.float32)
    for i, v in enumerate(special[:width]):
        a[(i * 7919) % width] = v
    b = np.sort(rs.randn(width).astype(np.float32))
    rows = np.stack([a, b, b[::-1]])
    guard = np.full(64, 123.0, np.float32)
    t = dev(ctx, np.concatenate([rows.reshape(-1), guard]))
    swd.sort_rows(ctx, t, 3, width)
    got = swd.download(ctx, t)
    assert np.array_equal(got[3 * width:], guard)
    assert np.array_equal(got[:3 * width].view(np.uint32).reshape(3, width), sorted_bits(rows))


def test_bad_sort_and_sum_arguments_are_refused(ctx):
    from rcgan_amd import _lib
    t = dev(ctx, np.zeros(64, np.float32))
    p = C.c_void_p(t.data_ptr())
    assert ctx.lib.rcgan_sort_rows_f32(ctx.h, 1, 48, p) == _lib.EINVALID_ARG
    assert ctx.lib.rcgan_sort_rows_f32(ctx.h, 0, 64, p) == _lib.EINVALID_ARG
    assert ctx.lib.rcgan_sort_rows_f32(ctx.h, 1, 64, None) == _lib.EINVALID_ARG
    assert ctx.lib.rcgan_absdiff_rowsum(ctx.h, 1, 64, 0, p, p, p, p) == _lib.EINVALID_ARG
    assert ctx.lib.rcgan_swd_moments(ctx.h, 1, 30, 32, 3, 0, 4, 1, p, p, p, p) == _lib.EINVALID_ARG          # 30 pixels
    assert ctx.lib.rcgan_swd_moments(ctx.h, 1, 32, 32, 3, 0, 1, 1, p, p, p, p) == _lib.EINVALID_ARG          # 676 positions
    assert ctx.lib.rcgan_swd_project(ctx.h, 1, 32, 32, 3, 0, 4, 1, p, p, p, 1, p, 48, p) == _lib.EINVALID_ARG


def test_row_sums_of_absolute_differences_stop_at_the_count(ctx):
    from rcgan_amd import swd
    rs = np.random.RandomState(3)
    a, b = rs.randn(6, 1024).astype(np.float32), rs.randn(6, 1024).astype(np.float32)
    a[:, 700:], b[:, 700:] = np.inf, np.inf
    count = np.array([700, 0, 300], np.int32)                                      # row r takes count[r mod 3]
    out = dev(ctx, np.full(7, -1.0))
    swd.absdiff_rowsum(ctx, dev(ctx, a), dev(ctx, b), dev(ctx, count), 6, 1024, out)
    got = swd.download(ctx, out)
    want = np.array([np.abs(a[r, :count[r % 3]].astype(np.float64) - b[r, :count[r % 3]]).sum() for r in range(6)])
    assert got[6] == -1.0 and np.abs(got[:6] - want).max() <= 1e-12 * max(want.max(), 1.0)


# ------------------------------------------------------------------------------------------------------------------ moments, projections
def image_set(shape, constant_channel=False):
    rs = np.random.RandomState(sum(shape))
    n, h, w, c = shape
    smooth = rs.randint(0, 256, size=(n, h // 4, w // 4, c)).repeat(4, axis=1).repeat(4, axis=2)
    x = np.clip(smooth + rs.randint(-20, 21, size=shape), 0, 255).astype(np.uint8)
    if constant_channel:
        x[..., 1] = 77
    return x


@pytest.mark.parametrize("shape, n_dir, constant", [((8, 32, 32, 3), 130, False), ((8, 28, 28, 1), 5, False), ((8, 28, 32, 3), 64, False),
                                                    ((8, 32, 32, 3), 7, True)])
def test_moments_and_projections_lie_within_the_derived_bound(ctx, shape, n_dir, constant):
    from rcgan_amd import swd
    x = image_set(shape, constant)
    n, h, w, c = shape
    dirs = swd.directions(n_dir, c, seed=11)
    segs = [(0, 3), (3, 8), (8, 8)]                                                # 3 and 5 images, and an empty third segment
    dx, d_dirs = dev(ctx, x), dev(ctx, dirs)
    off, wild = dev(ctx, np.array([0, 3, 8, 8], np.int32)), dev(ctx, np.array([-5, 3, 1000, 2], np.int32))   # (clamps to the same segments)
    worst = {}
    for level in range(3):
        n_pos = swd.positions(h, w, level)
        width = swd.pow2_at_least(5 * n_pos)
        mom = swd.swd_moments(ctx, dx, off, level)
        guard = torch.full((n_dir * 3 * width + 32,), 5.0, dtype=torch.float32, device=dx.device)
        proj = swd.swd_project(ctx, dx, off, mom, d_dirs[level], level, width, out=guard)
        again = swd.swd_project(ctx, dx, wild, swd.swd_moments(ctx, dx, wild, level), d_dirs[level], level, width)
        g_mom, g_proj, g_again = swd.download(ctx, mom, proj, again)
        assert (g_proj[n_dir * 3 * width:] == 5.0).all()
        g_proj = g_proj[:n_dir * 3 * width].reshape(n_dir, 3, width)
        assert g_again.tobytes() == g_proj.tobytes()
        assert not g_mom[2].any() and (g_proj[:, 2] == np.inf).all()
        for s, (lo, hi) in enumerate(segs[:2]):
            raw = SR.level_descriptors(x[lo:hi], level).reshape(-1, c)
            N, delta = len(raw), SR.DELTA[level]
            assert (np.abs(g_mom[s, :, 0] - raw.sum(axis=0)) <= N * delta + 1e-12 * np.abs(raw).sum(axis=0) + 1e-9).all()
            assert (np.abs(g_mom[s, :, 1] - (raw ** 2).sum(axis=0)) <= N * (510 * delta + delta ** 2) + 1e-12 * (raw ** 2).sum(axis=0) + 1e-9).all()
            m = (hi - lo) * n_pos
            want, bound = SR.projections(x[lo:hi], level, dirs[level]), SR.projection_bound(x[lo:hi], level, dirs[level])
            err = np.abs(g_proj[:, s, :m] - want)
            worst[level] = max(worst.get(level, 0.0), float((err / np.maximum(bound, 1e-30)).max()) if bound.max() > 0 else 0.0)
            print("shape %s level %d segment %d: max error %.3e, bound there %.3e, largest bound %.3e" %
                  (shape, level, s, err.max(), bound.reshape(-1)[err.argmax()], bound.max()))
            assert (err <= bound).all()
            assert (g_proj[:, s, m:] == np.inf).all()
        if constant:                                                               # the constant channel contributes exactly nothing
            alone = dirs[level].copy().reshape(n_dir, 49, c)
            alone[:, :, [0, 2]] = 0
            only = swd.download(ctx, swd.swd_project(ctx, dx, off, mom, dev(ctx, alone.reshape(n_dir, -1)), level, width))
            assert not only[:, 0, :3 * n_pos].any() and not only[:, 1, :5 * n_pos].any()
    print("shape %s: error / bound at most %s" % (shape, {l: round(v, 3) for l, v in worst.items()}))


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def world():
    from rcgan_amd import swd
    w = world_inputs()
    ev = swd.SwdEvaluator(K, directions=N_DIR)
    ev.prepare_real(w["real"], w["real_labels"])
    w.update(swd=swd, ev=ev, got=ev.evaluate(w["draw"], w["labels"]))
    yield w
    ev.close()


def as_ref(r):
    return dict(pooled=r["swd_levels"], per_class=r["per_class"])


def level_bounds(a, b, dirs):
    return np.array([1e3 * (SR.projection_bound(a, l, dirs[l]).max() + SR.projection_bound(b, l, dirs[l]).max()) for l in range(3)])


def test_the_evaluator_agrees_with_the_restatement_within_the_projection_bound(world):
    ev, got = world["ev"], world["got"]
    dirs = ev.host_dirs
    assert np.array_equal(dirs, world["swd"].directions(N_DIR, 3))
    ref = SR.evaluate(world["real"], world["real_labels"], world["draw"], world["labels"], K, dirs)
    n = len(world["draw"])
    bound = level_bounds(world["draw"], world["real"][:n], dirs)
    print("pooled %s against %s (bound %s)" % (got["swd_levels"], ref["pooled"], bound))
    assert (np.abs(got["swd_levels"] - ref["pooled"]) <= bound).all()
    assert (np.abs(got["floor_swd_levels"] - ref["floor_pooled"]) <= level_bounds(world["real"][:n], world["real"][n:2 * n], dirs)).all()
    g_rows = SR.first_rows(world["labels"], K, [PER_CLASS] * K)
    r_rows = SR.first_rows(world["real_labels"], K, [2 * PER_CLASS] * K)
    for c in range(K):
        a, b = world["draw"][g_rows[c]], world["real"][r_rows[c]]
        bound = level_bounds(a, b[:PER_CLASS], dirs)
        print("class %d: %s against %s (bound %s)" % (c, got["per_class"][c], ref["per_class"][c], bound))
        assert (np.abs(got["per_class"][c] - ref["per_class"][c]) <= bound).all()
        assert (np.abs(got["floor_per_class"][c] - ref["floor_per_class"][c]) <= level_bounds(b[:PER_CLASS], b[PER_CLASS:], dirs)).all()
    mean = got["per_class"].mean(axis=1)
    assert got["swd"] == pytest.approx(got["swd_levels"].mean(), rel=1e-15)
    assert got["intra_class_swd"] == pytest.approx(mean.mean(), rel=1e-15)
    assert got["intra_class_swd_se"] == pytest.approx(mean.std(ddof=1) / 2.0, rel=1e-12)
    assert np.allclose(got["intra_class_swd_levels"], got["per_class"].mean(axis=0), rtol=1e-15)
    assert got["images_used"].tolist() == [PER_CLASS] * K and got["classes_used"] == K and got["left_out"] == []
    assert (got["rejected_real"], got["rejected_generated"]) == (0, 0)
    again = ev.evaluate(world["draw"], world["labels"])
    for key in ("swd_levels", "per_class", "floor_swd_levels", "floor_per_class"):
        assert again[key].tobytes() == got[key].tobytes(), key


def test_the_four_orderings_hold_against_the_floor(world):
    ev, got = world["ev"], world["got"]
    shuffled = ev.evaluate(world["draw"], world["shuffled_labels"])
    collapsed, blurred = ev.evaluate(world["collapsed"], world["labels"]), ev.evaluate(world["blurred"], world["labels"])
    for name, r in (("clean", got), ("shuffled", shuffled), ("collapsed", collapsed), ("blurred", blurred)):
        print("%-9s pooled %s, intra-class %s, floor %s" % (name, np.round(r["swd_levels"], 1), np.round(r["intra_class_swd_levels"], 1),
                                                           np.round(r["floor_intra_class_swd_levels"], 1)))
    orderings(as_ref(got), as_ref(shuffled), as_ref(collapsed), as_ref(blurred))
    floor = dict(pooled=got["swd_levels"], per_class=got["floor_per_class"])        # the floor in the clean draw's place
    orderings(floor, as_ref(shuffled), as_ref(collapsed), as_ref(blurred))
    assert np.array_equal(shuffled["floor_per_class"], got["floor_per_class"])       # one count vector: the floor is kept
    assert len(ev.floors) == 1


def test_a_one_image_class_is_left_out_and_foreign_labels_are_counted(world):
    ev, labels = world["ev"], world["labels"].copy()
    rows3 = np.flatnonzero(labels == 3)
    labels[rows3[1:]] = K + 2
    r = ev.evaluate(world["draw"], labels)
    assert r["left_out"] == [3] and r["classes_used"] == K - 1 and np.isnan(r["per_class"][3]).all() and np.isnan(r["floor_per_class"][3]).all()
    assert r["rejected_generated"] == PER_CLASS - 1 and r["images_used"].tolist() == [PER_CLASS] * 3 + [0]
    assert np.array_equal(r["per_class"][:3], world["got"]["per_class"][:3])
    assert r["intra_class_swd"] == pytest.approx(r["per_class"][:3].mean(axis=1).mean(), rel=1e-15)
    json.dumps(world["swd"].json_ready(r))


def test_the_stand_alone_tool_prints_the_evaluators_numbers_as_one_json_line(world, tmp_path, capsys):
    a, b = os.path.join(str(tmp_path), "real.npz"), os.path.join(str(tmp_path), "generated.npz")
    np.savez(a, images=world["real"], labels=world["real_labels"])
    np.savez(b, images=world["draw"].transpose(0, 3, 1, 2).reshape(-1, 3072), labels=world["labels"])          # (both layouts are taken)
    world["swd"].main(["--real", a, "--generated", b, "--directions", str(N_DIR)])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    assert r["per_class"] == [[float(v) for v in row] for row in world["got"]["per_class"]] and r["swd"] == world["got"]["swd"]
    assert r["floor_intra_class_swd"] == world["got"]["floor_intra_class_swd"] and r["classes_used"] == K


def test_the_schedule_runs_the_metric_on_a_numpy_sampler(caplog):
    from rcgan_amd import metrics, train_cifar
    from rcgan_amd.cifar import Z_DIM
    FLAGS = train_cifar.define_flags().parse(["--swd_freq", "2", "--swd_samples", "200", "--swd_real_samples", "400", "--swd_directions", "16"])
    metrics.check_flags(FLAGS)
    train = (templates(41, np.arange(500) % 10).transpose(0, 3, 1, 2).reshape(-1, 3072), np.arange(500) % 10)
    sample = lambda labels, z: templates(int(abs(z[0, 0]) * 1e6) % 1000, labels).transpose(0, 3, 1, 2).reshape(-1, 3072) / 127.5 - 1.0
    plotted = []
    plot = type("Plot", (), dict(plot=staticmethod(lambda name, value: plotted.append((name, value)))))
    caplog.set_level(logging.INFO)
    E = metrics.Evaluations(FLAGS, 10, 0, "/nowhere", sample, np.random.RandomState(3), plot, np.zeros((100, Z_DIM), np.float32),
                            train_cifar.grid_labels(10), lambda: train, lambda: None)
    for iteration in range(2):
        E.run(iteration)
    E.close()
    lines = [r.getMessage() for r in caplog.records]
    assert [l for l in lines if "calculating" in l] == ["starting calculating sliced wasserstein distance.", "finished calculating sliced wasserstein distance."]
    assert "swd real set: 400 images, 16 directions per level" in lines
    assert sum(l.startswith("intra_class_swd: ") and "(10 of 10 classes), floor " in l for l in lines) == 1
    assert [n for n, _ in plotted] == ["swd", "intra_class_swd"] and all(np.isfinite(v) and v > 0 for _, v in plotted)
