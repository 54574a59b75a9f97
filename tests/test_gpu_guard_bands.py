"""The convolution, dense, batch-norm and head kernels inside guard bands (tests/guard.py): every arena tensor, every persistent buffer
(FakeParam values and gradients, moving statistics, loss scalars) and the workspace are framed by margins of 0xFF bytes -- NaN in every
float format -- and the case bodies of test_gpu_ops.py / test_gpu_many_classes_ops.py (their float64 oracles, unchanged) run inside:

  pass 1  the production-like 256 MiB workspace: the routes the models take;
  pass 2  a workspace of EXACTLY what the header's query function for the op returns (Context.group_wgrads off: one documented formula
          per call), so a query function smaller than its call's own check shows as RCGAN_EWORKSPACE_TOO_SMALL and a kernel that writes
          past the documented need damages the workspace's trailing margin.

After each pass: ctx.sync(), then Guard.check() -- every byte outside the bodies is still 0xFF.  A write outside a body damages a margin; a
read outside an input or of an unwritten output brings a NaN into a result the oracle comparison rejects (assert_close refuses non-finite
values); the direct ABI cases count the output elements that still hold the fill (Guard.unwritten).

Why each case reaches its route (line numbers: robust-conditional-gan_amd/csrc at the commit that added this file; those of the
filter gradient -- conv_wgrad.hip, conv_wgrad.h, api.hip:166-170 -- at the commit that gave it its own translation unit):

  route                                  case (field order of the list it comes from)      reached because
  -------------------------------------  ------------------------------------------------  ------------------------------------------------
  conv, scalar / direct                  (2,9,7,3,5,3,1) (3,7,7,6,4,5,2,relu)              not mfma_eligible (conv_mfma.hip:1603: channels % 64 != 0, or
                                         (2,4,4,5,3,5,2) (2,28,28,1,8,5,2)                 5x5 / stride 2), img_side 0 (conv_image.hip:19) and every
                                                                                           small_*_kind 0 (conv_small.hip:325-342: no 128- / 256-channel
                                                                                           side) -> direct_fwd / direct_dgrad / direct_wgrad, the last
                                                                                           branches of rcgan_conv2d_fwd_residual (api.hip:907),
                                                                                           _bwd_data_residual (:958) and conv_wgrad_off_mfma (:170), any dtype
  conv, 64x64 matrix-core tiles          (3,5,5,64,128,3,1,relu) (3,5,5,128,64,1,1)        16-bit, channels % 64 == 0 -> mfma_eligible; M = 75 pixels = one
                                         (3,5,5,128,128,3,1,relu): not in CONV_CASES       256-pixel tile, far below the 190 / 200 / 384 workgroups the
                                                                                           larger tiles ask for: mfma_conv_route returns CR_64
                                                                                           (conv_mfma.hip:1818), whose second tile has an 11-pixel tail,
                                                                                           forward and data gradient.  Filter gradient: the first two are
                                                                                           not mfma_wgrad_eligible (conv_wgrad.hip:810: cin, cout % 128) and take
                                                                                           direct_wgrad (api.hip:170); the 128 -> 128 sibling is, and with
                                                                                           M % 32 != 0 wgrad3_geom refuses it (:820): mfma_wgrad_choose
                                                                                           (:943) returns the per-tap kernel, 75-pixel tail included
  conv, folded upsample / sub-pixel      (1,8,8,128,256,3,1,up) (32,8,8,256,128,3,1,up,    IN_UPSAMPLE2X: rcgan_conv2d_bwd_data_residual (api.hip:933)
                                         relu)                                             needs the full-resolution scratch unless posed in gather form;
                                                                                           wgrad_pose (conv_wgrad.hip:1076) takes mfma_wgrad_sub_kind = 1 for the second
                                                                                           (n*4*4 % 32 == 0) and 0 for the first (16 pixels): the plain
                                                                                           pose rcgan_conv_workspace_bytes promises and the sub-pixel one
  conv, image end (conv_image.hip)       (4,32,32,3,128,3,1) (3,16,16,256,3,3,1)           16-bit, W in {8,16,32}, h*w >= 256, <= 3 channels on one side and
                                         (2,32,8,3,256,3,1) (5,16,32,128,2,3,1,relu)       128 / 256 on the other: img_side != 0 (conv_image.hip:19-27) ->
                                                                                           img_fwd (api.hip:903), img_dgrad (:951), img_wgrad (:166); the
                                                                                           IN_RELU case's data gradient has a mask and no small kind:
                                                                                           direct_dgrad (:958)
  conv, small side (conv_small.hip)      the four above in fp32, and                       img_side needs 16-bit, so in fp32 small_fwd_kind /
                                         (3,10,6,128,3,3,1,relu) in every dtype            small_dgrad_kind / small_wgrad_kind (conv_small.hip:325-342: <= 4
                                                                                           channels against 128 / 256, 1x1 / 3x3, stride 1) send them to
                                                                                           small_fwd (api.hip:904), small_dgrad (:954), small_wgrad (:168);
                                                                                           W = 6 is no power of two (conv_image.hip:23), so that case takes
                                                                                           small_fwd kind 2 and small_wgrad kind 2 in 16-bit too; IN_RELU
                                                                                           rules out small_dgrad (conv_small.hip:332): direct_dgrad
  conv, nine-tap filter gradient         (3,16,8,128,128,3,1) (40,8,8,128,128,3,1,relu)    mfma_wgrad_eligible (cin, cout % 128 == 0); RCGAN_WGRAD9_MINWORK =
                                         (2,16,16,128,128,3,1,relu)                        RCGAN_WGRAD9_GROUP_MINWORK = 0 (the switches of
                                         (6,16,16,256,256,3,1,up): its sub-pixel form      test_conv2d_fwd_bwd_nine_tap_forced) put the nine-tap kernel on
                                         grouped and single                                offer: mfma_wgrad_choose (conv_wgrad.hip:935-943) returns WK_NINE
                                                                                           where mfma_wgrad9_takes (conv_wgrad9.hip:385: 3x3, W 8 / 16 / 32,
                                                                                           M % 128 == 0, sub-pixel forms M % 64 == 0) -- single through
                                                                                           mfma_wgrad_launch (:968), grouped through the planner
                                                                                           (:1216, :1295, mfma_wgrad9_group_launch :1341).  The
                                                                                           fallback at conv_wgrad.hip:976 cannot be reached from
                                                                                           rcgan_conv2d_bwd_weight: the entry check (:1132) asks for
                                                                                           mfma_wgrad_ws_need, whose 1024 * cout spare floats (conv_wgrad.h:50)
                                                                                           exceed the second bias tail of at most 128 chunks x cout, so at
                                                                                           or above the call's own need the nine-tap slabs always fit and
                                                                                           both passes run the nine-tap kernel
  direct filter gradient of 64-channel   (6,8,8,64,128,3,1,relu) (8,4,8,64,128,3,1)        cin = 64: not mfma_wgrad_eligible, whatever the switches say ->
  layers (forward, dgrad: CR_64)         (4,2,16,64,256,3,1,relu), grouped and single      direct_wgrad alone (api.hip:170) and from the group (conv_wgrad.hip:1336)
  conv, 256x256 eight-wave kernels       (52,32,32,64,256,3,1,relu)                        Cout % 256 == 0 and 208 / 200 tiles of 256 pixels >= p8_min = 200
                                         (50,32,32,256,256,1,1): both directions           (conv_mfma.hip:1813): CR_H8 / CR_P8 (the halo form takes 3x3 only);
                                                                                           the smallest entries of CONV_CASES past that count
  conv, halo-patch 256x256 / 256x128     (52,32,32,256,256,3,1,relu)                       ditto, forward and data gradient (Cin = Cout = 256); Cout = 128:
                                         (50,32,32,128,128,3,1,relu)                       200 tiles >= p8n_min = 190 -> CR_H8N (conv_mfma.hip:1814)
  ConvMeanPool                           (4,32,32,128,128,True,True), force9 both          OUT_MEANPOOL2: mfma_pool_ok; force9 = the two switches above
  residual from half resolution          (4,16,16,64,128)                                  RESID_UPSAMPLE2X: rcgan_conv_resid_up_ok (api.hip:693)
  accumulate, forced direct              test_conv_accumulate_and_force_direct             CONV_ACCUMULATE / CONV_FORCE_DIRECT flags
  register-filter conv                   (3,16,True,False) (5,16,True,False)               rcgan_conv_rf_ok asserted by the body
  8x8 stage                              test_d_trunk_equals_layerwise_blocks, n = 3       ops.d_trunk is called by the body
  pooled boundary                        (6,"NEG_MEAN",None)                               ops.d_trunk(pool=ACT_RELU) is called by the body
  grouped filter gradients               grouped_filter_gradients_case                     rcgan_conv2d_bwd_weight_group is called by the body
  dense                                  (5,110,1024) (7,128,1) (9,300,128) (4,3072,10)    rcgan_linear_* (ops.linear: sigma set -> never the conv route)
  dense on the matrix cores              (40,64,1024)                                      ops.linear:648 (16-bit, no sigma, k % 64 == n % 64 == 0, n >= 1024)
  transposed conv                        (7,10,6) (14,138,1)                               rcgan_deconv2d_* are called by ops.deconv2d
  label-column filter gradient           (9,4,128,3,64,3) (2,14,64,16,128,5)               ops.deconv2d:630 (c1 >= 64, c2 <= 16, cout >= 64, ow <= 32)
  BN_COLUMN                              ((6,4,4,64),T) ((5,4,4,128),T) ((130,4,4,64),T)   bn_fused_ok: c a power of two in 64 .. 2048 (bn_plan.h:129);
                                         ((3,32,32,64),T) ((16,1024),F)                    rows * c below the tree threshold
  BN_VEC                                 ((3,3,3,200),T) ((4,5,5,72),F) ((3,5,5,24),T)     c % 8 == 0, not a power of two >= 64, and the workspace holds the
                                                                                           tables (bn_plan.h:153) -- in both passes, or the apply would fall
                                                                                           to the scalar kernels without a word
  BN_SCALAR                              ((3,5,5,20),T)                                    c % 8 != 0 (bn_plan.h:154); c = 24 of test_batch_norm's list is a
                                                                                           vector case by that line, so 20 stands in for the scalar route
  BN_TREE                                ((32,32,32,128),T) ((64,16,16,256),F)             rows * c = 4 Mi >= RCGAN_BN_TREE_MIN (tests/conftest.py), bn_tree_ok
  BN_WIDE                                K = 17: (17,128,4) and (17,20,4)                  n_labels > MAX_LABELS = 16 (bn_plan.h:41); c = 20: c % 8 != 0 ->
                                                                                           bn_partial_kernel
  segmented                              (5,(2,8,8,64))                                    bn_choose (bn_plan.h:141-154): c = 64 fused, 5 x 1 counter lines
                                                                                           -> BN_COLUMN with the segment as grid z (:151), statistics and apply
                                         (3,(2,4,4,24)) (3,(2,3,3,200))                    not fused -> one segment at a time (:141, :143), each BN_VEC
                                                                                           (c % 8 == 0, :153; the list's comment calls c = 24 scalar: it is not)
                                         (9,(1,2,2,2048))                                  9 x 32 > 256 counter lines: statistics one segment at a time
                                                                                           (:141), each BN_COLUMN; the apply keeps the segmented BN_COLUMN (:143)
  inference                              test_batch_norm_infer                             rcgan_bn_infer
  head                                   HEAD_CASES n = 12 and n = 16; pooled (16,8,64,    rcgan_proj_head_fwd_bwd; v = 17 > HEAD_MAX_V -> head_wide
                                         128); test_head_and_losses; v = 17                (loss.hip:783)
  unfused head, losses, softmax rows,    tests/test_gpu_head_loss_edges.py (runs guarded   the C entry points of loss.hip outside the fused head and
  inference batch norm and its adjoint   itself: its own module fixtures and case lists)   rcgan_bn_infer / rcgan_bn_infer_bwd, called directly

fp32, bf16 and fp16 contexts; the chip-filling convolution cases and the grouped filter gradients (bf16 descriptors) run on bf16 only, the
head cases that are fp32 whatever the activation type on the fp32 context only.

Workspace sizes of pass 2: rcgan_conv_workspace_bytes (convolutions, transposed convolutions), rcgan_conv2d_bwd_weight_group_workspace_bytes,
rcgan_deconv2d_bwd_weight_concat_bytes, rcgan_linear_workspace_bytes, rcgan_bn_workspace_bytes_labels (x nseg for the segmented calls),
rcgan_proj_head_workspace_bytes, rcgan_softmax_xent_workspace_bytes, rcgan_recover_mse_workspace_bytes; 0 bytes for the ops that take no
workspace.
"""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_classifier_ops as K
from tests import test_gpu_many_classes_ops as M
from tests import test_gpu_ops as T
from tests.guard import guarded
from tests.gpu_util import assert_close, half_round, make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _contexts():
    """One guarded context per activation dtype, made on first use and kept for the module."""
    made = {}

    def get(mode):
        if mode not in made:
            ctx = make_ctx(mode, arena=1 << 20)          # (its own arena is replaced by the guarded one)
            cm = guarded(ctx)
            ctx.guard = cm.__enter__()
            made[mode] = (ctx, cm)
        return made[mode][0], mode

    yield get
    for ctx, cm in made.values():
        cm.__exit__(None, None, None)
        ctx.close()


@pytest.fixture(scope="module", params=["f32", "bf16", "f16"])
def dev(request, _contexts):
    return _contexts(request.param)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def dev16(request, _contexts):
    """The matrix-core kernels run on 16-bit activations only."""
    return _contexts(request.param)


@pytest.fixture(scope="module")
def devbf16(_contexts):
    """The chip-filling cases, and the body that makes its own bf16 descriptors."""
    return _contexts("bf16")


@pytest.fixture(scope="module")
def dev32(_contexts):
    """The head is fp32 whatever the activation dtype."""
    return _contexts("f32")


def test_the_guard_is_in_place(dev):
    """The context the cases run in is the guarded one, and the fill is what the DEVICE holds: a fresh tensor is all pattern, an uploaded one
    has none left, a zero-filled persistent buffer neither, and nothing outside them has changed."""
    from rcgan_amd import _lib as L
    from tests import guard as G
    ctx, _ = dev
    g = ctx.guard
    g.clear()
    assert isinstance(ctx.arena, G.GuardedArena) and ctx.ws_bytes == G.WS_DEFAULT and ctx.ws_ptr == g.ws.ptr and ctx.ws_ptr % 256 == 0
    t = ctx.empty((5, 7, 3))
    assert g.unwritten(t) == t.size and not np.isfinite(ctx.download(t)).any()
    ctx.upload(np.ones((5, 7, 3), np.float32), out=t)
    p = ctx.persistent((9,), L.F32, fill=0.0)
    q = ctx.persistent((4,), "i32")
    assert g.unwritten(t) == 0 and g.unwritten(p) == 0 and g.unwritten(q) == 4 and (ctx.download(q) == -1).all()
    with g.workspace(1000):
        assert ctx.ws_bytes == 1000 and ctx.ws_ptr % 256 == 0 and ctx.ws_ptr != g.ws_default.ptr
    ctx.sync()
    g.check()


def _both_passes(dev, need, body, grouped=None):
    """body() with the production-like workspace, then inside a workspace of exactly `need` bytes with one filter gradient per call
    (grouped: keep that setting of Context.group_wgrads in both passes instead); bands checked after each."""
    ctx, _ = dev
    g = ctx.guard
    keep = ctx.group_wgrads
    try:
        for tight in (False, True):
            g.clear()
            ctx.group_wgrads = grouped if grouped is not None else (False if tight else keep)
            if tight:
                with g.workspace(need):
                    body()
                    ctx.sync()
                    g.check()
            else:
                body()
                ctx.sync()
                g.check()
    finally:
        ctx.group_wgrads = keep


def _conv_desc(ctx, case):
    from rcgan_amd import _lib as L
    n, h, w, cin, cout, k, s, up, relu = case
    return L.ConvDesc(n, h, w, cin, cout, k, k, s, ctx.act_dtype, (L.CONV_IN_UPSAMPLE2X if up else 0) | (L.CONV_IN_RELU if relu else 0))


def _conv_need(ctx, *cases):
    return max(ctx.lib.rcgan_conv_workspace_bytes(C.byref(_conv_desc(ctx, c))) for c in cases)


def _case(n, h, w, cin, cout, k, s, *flags):
    c = (n, h, w, cin, cout, k, s, "up" in flags, "relu" in flags)
    assert c in T.CONV_CASES, c
    return c


# ---------------------------------------------------------------------------------------------------- convolution
CONV_BOTH = [_case(2, 9, 7, 3, 5, 3, 1), _case(3, 7, 7, 6, 4, 5, 2, "relu"), _case(2, 4, 4, 5, 3, 5, 2), _case(2, 28, 28, 1, 8, 5, 2),
             _case(3, 5, 5, 64, 128, 3, 1, "relu"), (3, 5, 5, 128, 64, 1, 1, False, False), (3, 5, 5, 128, 128, 3, 1, False, True),
             _case(1, 8, 8, 128, 256, 3, 1, "up"), _case(32, 8, 8, 256, 128, 3, 1, "up", "relu"),
             _case(4, 32, 32, 3, 128, 3, 1), _case(3, 16, 16, 256, 3, 3, 1), _case(3, 10, 6, 128, 3, 3, 1, "relu"),
             _case(5, 16, 32, 128, 2, 3, 1, "relu"), _case(2, 32, 8, 3, 256, 3, 1)]
CONV_BIG = [_case(52, 32, 32, 64, 256, 3, 1, "relu"), _case(50, 32, 32, 256, 256, 1, 1), _case(52, 32, 32, 256, 256, 3, 1, "relu"),
            _case(50, 32, 32, 128, 128, 3, 1, "relu")]
NINE_TAP = [_case(3, 16, 8, 128, 128, 3, 1), _case(40, 8, 8, 128, 128, 3, 1, "relu"), _case(2, 16, 16, 128, 128, 3, 1, "relu"),
            _case(6, 16, 16, 256, 256, 3, 1, "up"),
            # cin = 64: the direct filter gradient under the same switches, alone and out of the group
            _case(6, 8, 8, 64, 128, 3, 1, "relu"), _case(8, 4, 8, 64, 128, 3, 1), _case(4, 2, 16, 64, 256, 3, 1, "relu")]
assert all(c in T.WGRAD9_CASES for c in NINE_TAP)


@pytest.mark.parametrize("case", CONV_BOTH)
def test_conv2d(dev, case):
    ctx, _ = dev
    _both_passes(dev, _conv_need(ctx, case), lambda: T.test_conv2d_fwd_bwd(dev, case))


@pytest.mark.parametrize("case", CONV_BIG)
def test_conv2d_chip_filling_kernels(devbf16, case):
    ctx, _ = devbf16
    _both_passes(devbf16, _conv_need(ctx, case), lambda: T.test_conv2d_fwd_bwd(devbf16, case))


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("case", NINE_TAP)
def test_conv2d_nine_tap_forced(dev16, case, grouped, monkeypatch):
    ctx, _ = dev16
    monkeypatch.setenv("RCGAN_WGRAD9_MINWORK", "0")
    monkeypatch.setenv("RCGAN_WGRAD9_GROUP_MINWORK", "0")
    d = _conv_desc(ctx, case)
    need = ctx.lib.rcgan_conv2d_bwd_weight_group_workspace_bytes(1, C.byref(d)) if grouped else _conv_need(ctx, case)
    assert need >= _conv_need(ctx, case)
    _both_passes(dev16, need, lambda: T.test_conv2d_fwd_bwd(dev16, case), grouped=grouped)


@pytest.mark.parametrize("force9", [False, True])
def test_conv2d_meanpool(dev16, force9, monkeypatch):
    from rcgan_amd import _lib as L
    ctx, _ = dev16
    case = (4, 32, 32, 128, 128, True, True)
    n, h, w, cin, cout, relu, _ = case
    d = L.ConvDesc(n, h, w, cin, cout, 3, 3, 1, ctx.act_dtype, L.CONV_OUT_MEANPOOL2 | L.CONV_IN_RELU)
    # (n = 4: the body takes the one-layer entry point in both passes)
    _both_passes(dev16, ctx.lib.rcgan_conv_workspace_bytes(C.byref(d)), lambda: T.test_conv2d_meanpool(dev16, case, force9, monkeypatch))


def test_conv_residual_from_half_resolution(dev):
    from rcgan_amd import _lib as L
    ctx, _ = dev
    case = (4, 16, 16, 64, 128)
    d = L.ConvDesc(4, 16, 16, 64, 128, 3, 3, 1, ctx.act_dtype, 0)
    _both_passes(dev, ctx.lib.rcgan_conv_workspace_bytes(C.byref(d)), lambda: T.test_conv_residual_from_half_resolution(dev, case))


def test_conv_accumulate_and_force_direct(dev):
    _both_passes(dev, 0, lambda: T.test_conv_accumulate_and_force_direct(dev))           # forward only: no workspace


@pytest.mark.parametrize("n", [3, 5])
def test_register_filter_conv(dev16, n):
    ctx, _ = dev16
    need = _conv_need(ctx, (n, 16, 16, 128, 128, 3, 1, False, True))
    _both_passes(dev16, need, lambda: T.test_register_filter_conv_equals_tile_kernels(dev16, n, 16, True, False))


def test_d_trunk(dev16):
    ctx, _ = dev16
    need = _conv_need(ctx, (3, 8, 8, 128, 128, 3, 1, False, True))
    _both_passes(dev16, need, lambda: T.test_d_trunk_equals_layerwise_blocks(dev16, 3))


def test_d_trunk_pooled_boundary(dev16):
    ctx, _ = dev16
    need = max(_conv_need(ctx, (6, 8, 8, 128, 128, 3, 1, False, True)), ctx.lib.rcgan_proj_head_workspace_bytes(6, 128, 10))
    _both_passes(dev16, need, lambda: T.test_d_trunk_pooled_boundary(dev16, 6, "NEG_MEAN", None))


def test_grouped_filter_gradients(devbf16):
    """The grouped call with the workspace its own query function returns (the single calls of the body need less), and every filter /
    bias gradient of both written in full."""
    ctx, _ = devbf16
    g = ctx.guard
    descs = T.grouped_filter_gradient_descs()
    arr = (type(descs[0]) * len(descs))(*descs)
    need = ctx.lib.rcgan_conv2d_bwd_weight_group_workspace_bytes(len(descs), arr)
    assert need >= 2 * max(ctx.lib.rcgan_conv_workspace_bytes(C.byref(d)) for d in descs)
    for tight in (False, True):
        g.clear()
        if tight:
            with g.workspace(need):
                items = T.grouped_filter_gradients_case(ctx)
                ctx.sync()
                g.check()
        else:
            items = T.grouped_filter_gradients_case(ctx)
            ctx.sync()
            g.check()
        for _, _, _, dws, dbs in items:
            for t in dws + [b for b in dbs if b is not None]:
                assert g.unwritten(t) == 0


# ---------------------------------------------------------------------------------------------------- dense / transposed convolution
@pytest.mark.parametrize("m,k,n", [(5, 110, 1024), (7, 128, 1), (9, 300, 128), (4, 3072, 10)])
def test_linear(dev, m, k, n):
    ctx, _ = dev
    _both_passes(dev, ctx.lib.rcgan_linear_workspace_bytes(m, k, n), lambda: T.test_linear(dev, m, k, n))


def test_wide_dense_layer_on_the_matrix_cores(dev16, monkeypatch):
    ctx, _ = dev16
    m, k, n = 40, 64, 1024
    need = max(ctx.lib.rcgan_linear_workspace_bytes(m, k, n), _conv_need(ctx, (m, 1, 1, k, n, 1, 1, False, False)))
    _both_passes(dev16, need, lambda: T.test_wide_dense_layer_on_the_matrix_cores(dev16, m, k, n, monkeypatch))


@pytest.mark.parametrize("hin,cin,cout", [(7, 10, 6), (14, 138, 1)])
def test_deconv(dev, hin, cin, cout):
    from rcgan_amd import _lib as L
    ctx, _ = dev
    d = L.ConvDesc(3, 2 * hin, 2 * hin, cout, cin, 5, 5, 2, ctx.act_dtype, 0)           # ops.deconv2d's descriptor: the conv it transposes
    _both_passes(dev, ctx.lib.rcgan_conv_workspace_bytes(C.byref(d)), lambda: T.test_deconv(dev, hin, cin, cout))


@pytest.mark.parametrize("n,hin,c1,c2,cout,k", [(9, 4, 128, 3, 64, 3), (2, 14, 64, 16, 128, 5)])
def test_deconv_filter_gradient_with_label_columns(dev, n, hin, c1, c2, cout, k):
    from rcgan_amd import _lib as L
    ctx, _ = dev
    d = L.ConvDesc(n, 2 * hin, 2 * hin, cout, c1 + c2, k, k, 2, ctx.act_dtype, 0)
    need = ctx.lib.rcgan_deconv2d_bwd_weight_concat_bytes(C.byref(d), c1)
    _both_passes(dev, need, lambda: T.test_deconv_filter_gradient_with_label_columns(dev, n, hin, c1, c2, cout, k))


# ---------------------------------------------------------------------------------------------------- batch norm
BN_CASES = [((6, 4, 4, 64), True), ((5, 4, 4, 128), True), ((130, 4, 4, 64), True), ((3, 32, 32, 64), True), ((16, 1024), False),      # column
            ((3, 3, 3, 200), True), ((4, 5, 5, 72), False),                                                                           # vector
            ((3, 5, 5, 24), True),
            ((3, 5, 5, 20), True),                                                                                                    # scalar
            ((32, 32, 32, 128), True), ((64, 16, 16, 256), False)]                                                                    # tree


@pytest.mark.parametrize("shape,cond", BN_CASES)
def test_batch_norm(dev, shape, cond):
    ctx, _ = dev
    rows = int(np.prod(shape[:-1]))
    need = ctx.lib.rcgan_bn_workspace_bytes_labels(rows, shape[-1], 10 if cond else 1)
    _both_passes(dev, need, lambda: T.test_batch_norm(dev, shape, cond))


@pytest.mark.parametrize("c", [128, 20])
def test_batch_norm_wide_labels(dev, c):
    ctx, _ = dev
    K, n, rps = 17, 4, 16
    _both_passes(dev, ctx.lib.rcgan_bn_workspace_bytes_labels(n * rps, c, K), lambda: M.test_cond_bn_many_classes(dev, K, c, n))


@pytest.mark.parametrize("nseg,shape", T.BN_SEGMENT_CASES)
def test_batch_norm_segments(dev, nseg, shape):
    ctx, _ = dev
    n, h, w, c = shape
    need = nseg * ctx.lib.rcgan_bn_workspace_bytes_labels(n * h * w, c, 10)
    _both_passes(dev, need, lambda: T.test_batch_norm_segments_routes(dev, nseg, shape))


def test_batch_norm_infer(dev):
    _both_passes(dev, 0, lambda: T.test_batch_norm_infer(dev))


# ---------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("case", sorted(T.HEAD_CASES, key=lambda c: c[:2])[:2])
def test_proj_head(dev32, case):
    ctx, _ = dev32
    _both_passes(dev32, ctx.lib.rcgan_proj_head_workspace_bytes(case[0], 128, 10), lambda: T.test_proj_head(dev32, case))


def test_proj_head_pools_features(dev):
    ctx, _ = dev
    case = (16, 8, 64, 128, "HINGE_REAL", "HINGE_FAKE")
    _both_passes(dev, ctx.lib.rcgan_proj_head_workspace_bytes(16, 128, 10), lambda: T.test_proj_head_pools_features(dev, case))


def test_head_and_losses(dev):
    ctx, _ = dev
    need = max(ctx.lib.rcgan_linear_workspace_bytes(6, 300, 128), ctx.lib.rcgan_linear_workspace_bytes(6, 128, 1))
    _both_passes(dev, need, lambda: T.test_head_and_losses(dev))


@pytest.mark.parametrize("spec", M.HEAD_PARTS)
def test_proj_head_many_classes(dev32, spec):
    ctx, _ = dev32
    _both_passes(dev32, ctx.lib.rcgan_proj_head_workspace_bytes(32, 128, 17), lambda: M.test_proj_head_many_classes(dev32, 17, spec))


# ---------------------------------------------------------------------------------------------------- losses with a workspace of their own
@pytest.mark.parametrize("rows,cols", [(7, 10), (130, 100)])
def test_softmax_xent(dev32, rows, cols):
    """rcgan_softmax_xent_fwd_bwd through the C ABI against test_gpu_classifier_ops' float64 restatement, in both workspaces."""
    from rcgan_amd import _lib as L
    ctx, _ = dev32
    g = ctx.guard
    x, lab = K._xent_case(rows, cols, rows * 7 + cols)
    L_ref, d_ref, n_ref = K._xent_ref(x, lab, 0.75)
    p = lambda t: C.c_void_p(t.ptr)

    def body():
        ctx.new_step()
        xd, labd, dl = ctx.upload(x, L.F32), ctx.upload(lab), ctx.empty((rows, cols), L.F32)
        loss, ncor = ctx.persistent((1,), L.F32, fill=0.0), ctx.persistent((1,), L.F32, fill=0.0)
        ctx.check(ctx.lib.rcgan_softmax_xent_fwd_bwd(ctx.h, rows, cols, p(xd), p(labd), 0.75, p(loss), p(ncor), p(dl), C.c_void_p(ctx.ws_ptr),
                                                     ctx.ws_bytes))
        ctx.sync()
        assert g.unwritten(dl) == 0
        assert abs(float(ctx.download(loss)[0]) - L_ref) <= 2e-5 * max(1.0, abs(L_ref)) and float(ctx.download(ncor)[0]) == n_ref
        assert_close(ctx.download(dl), d_ref, 2e-5, "dlogits")

    _both_passes(dev32, ctx.lib.rcgan_softmax_xent_workspace_bytes(rows), body)


def test_recover_mse(dev):
    """rcgan_recover_mse_fwd_bwd (kernel comment, loss.hip:568): loss = mean_r sum_y yrec[r,y] * mean_pix (actual[r] - gen[r,y])^2 with its
    gradients, against float64 of the same formula on inputs rounded to the activation format; 784 pixels = three rounds of 256 and a tail.
    fp32 sums of fp32 products: 2e-5; dgen is stored in the activation format: its storage bound."""
    from rcgan_amd import _lib as L
    ctx, mode = dev
    g = ctx.guard
    r, ydim, pix = 3, 10, 784
    rs = np.random.RandomState(31)
    gen, act = half_round(mode, rs.rand(r * ydim, pix)), half_round(mode, rs.rand(r, pix))
    yrec = rs.dirichlet(np.ones(ydim), size=r).astype(np.float32)
    d = gen.astype(np.float64).reshape(r, ydim, pix) - act.astype(np.float64)[:, None, :]
    sq = (d * d).mean(2)
    loss_ref, dyrec_ref = (sq * yrec).sum() / r, sq / r
    dgen_ref = (2.0 * d / pix * yrec[:, :, None] / r).reshape(r * ydim, pix)
    p = lambda t: C.c_void_p(t.ptr)

    def body():
        ctx.new_step()
        gd, ad, yd = ctx.upload(gen), ctx.upload(act), ctx.upload(yrec, L.F32)
        dgen, dyrec, loss = ctx.empty(gen.shape), ctx.empty((r, ydim), L.F32), ctx.persistent((1,), L.F32)
        ctx.check(ctx.lib.rcgan_recover_mse_fwd_bwd(ctx.h, r, ydim, pix, gd.dtype, p(gd), p(ad), p(yd), p(loss), p(dgen), p(dyrec),
                                                    C.c_void_p(ctx.ws_ptr), ctx.ws_bytes))
        ctx.sync()
        assert g.unwritten(dgen) == 0 and g.unwritten(dyrec) == 0 and g.unwritten(loss) == 0
        assert_close(ctx.download(loss), np.array([loss_ref]), 2e-5, "recover loss")
        assert_close(ctx.download(dyrec), dyrec_ref, 2e-5, "recover dyrec")
        assert_close(ctx.download(dgen), dgen_ref, T.TOL[mode], "recover dgen")

    _both_passes(dev, ctx.lib.rcgan_recover_mse_workspace_bytes(r, ydim), body)
