/*
 * rcgan_hip.h -- flat C ABI of librcgan_hip.so: the MI355X (gfx950) kernels behind the RCGAN
 * generator/discriminator training step.
 *
 * The reference (tkkiran/Robust-Conditional-GAN) has no FFI / custom-op seam: every FLOP is a stock
 * TensorFlow-1.5 kernel reached through its L1 Python op wrappers.  This ABI sits directly under an
 * L1-compatible Python shim (robust-conditional-gan_amd/ops_mnist.py, ops_cifar.py); each entry point
 * names the reference call site whose TF kernel it replaces (paths relative to the reference root).
 *
 * Conventions:
 *   - every entry returns int: 0 = ok, <0 = RCGAN_E*; rcgan_last_error(ctx) gives the message.
 *     No exceptions or aborts cross the ABI.
 *   - all buffers are caller-owned DEVICE pointers; the library never frees or retains them past the
 *     call.  Scratch is a caller-provided workspace (see the *_workspace_bytes helpers).
 *   - one hipStream_t per ctx; every call is asynchronous on that stream; a ctx is not thread-safe;
 *     distinct ctxs are independent (one ctx per rank/process).
 *   - activations are NHWC; conv filters HWIO ([kh][kw][Cin][Cout]); transposed-conv filters
 *     [kh][kw][Cout][Cin] (mnist/ops.py:74).  Parameters, their gradients and optimiser state are
 *     always fp32; activations / activation gradients are fp32 or bf16 (desc.dtype).
 */
#ifndef RCGAN_HIP_H
#define RCGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCGAN_OK 0
#define RCGAN_EINVALID_ARG (-1)
#define RCGAN_EUNSUPPORTED_SHAPE (-2)
#define RCGAN_EWORKSPACE_TOO_SMALL (-3)
#define RCGAN_EHIP (-4)
#define RCGAN_ERCCL (-5)

#define RCGAN_F32 0
#define RCGAN_BF16 1
#define RCGAN_F16 2   /* IEEE half: only in the fp16 build of the library (librcgan_hip_f16.so), which has no bf16 */

/* activation codes shared by several entry points */
#define RCGAN_ACT_NONE 0
#define RCGAN_ACT_RELU 1
#define RCGAN_ACT_LRELU 2   /* tf.maximum(x, 0.2x): mnist/ops.py:94-95 */
#define RCGAN_ACT_TANH 3
#define RCGAN_ACT_SIGMOID 4

typedef struct rcgan_ctx rcgan_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* stream: a hipStream_t owned by the caller (e.g. torch.cuda.current_stream().cuda_stream) or NULL
 * for the null stream.  Replaces: tf.Session(config) at cifar10/gan_resnet.py:494-496, mnist/main.py:100. */
int rcgan_create(rcgan_ctx** out, int device, void* stream);
int rcgan_destroy(rcgan_ctx* ctx);
const char* rcgan_last_error(rcgan_ctx* ctx);
const char* rcgan_version(void);
/* The 16-bit activation dtype this build of the library computes in: RCGAN_BF16 (librcgan_hip.so) or RCGAN_F16
 * (librcgan_hip_f16.so, the same sources compiled with -DRCGAN_HALF_FP16=1: v_mfma_f32_16x16x32_f16, v_cvt_f16_f32).
 * The other 16-bit dtype is rejected with RCGAN_EINVALID_ARG.  (The reference computes in fp32; BASELINE configs 3 / 5.) */
int rcgan_half_dtype(void);
/* CRC-32C (Castagnoli, reflected 0x82F63B78), host-side, no GPU needed: crc of `n` bytes continuing from `crc`
 * (pass 0 to start).  The checksum TensorFlow's V2 checkpoint bundles carry per tensor and per table block
 * (tf.train.Saver at cifar10/gan_resnet.py:906, mnist/model.py:265); used by the bundle reader/writer of the host layer. */
unsigned rcgan_crc32c(unsigned crc, const void* data, size_t n);
int rcgan_set_stream(rcgan_ctx* ctx, void* stream);
/* Fork/join onto the context's second stream: launches between side_begin and side_end run on it, ordered after
 * everything issued before the fork; side_join makes the main stream wait for them.  Used to run a layer's filter
 * gradient next to its data gradient (two sess.run-internal independent TF ops: conv2d_backprop_filter /
 * conv2d_backprop_input).  Works under rcgan_graph_begin/end (becomes a fork/join in the captured graph). */
int rcgan_side_begin(rcgan_ctx* ctx);
int rcgan_side_end(rcgan_ctx* ctx);
int rcgan_side_join(rcgan_ctx* ctx);
int rcgan_stream_sync(rcgan_ctx* ctx);
/* HIP-event timing on the ctx stream (bench.py roofline leg): slot in [0,64). */
int rcgan_event_record(rcgan_ctx* ctx, int slot);
int rcgan_event_elapsed_ms(rcgan_ctx* ctx, int slot_start, int slot_end, float* ms);
/* Per-kernel profiling: while armed, every launch of the chosen kernel is bracketed by HIP events on the ctx
 * stream (eager launches only, not graph replays).  rcgan_prof_end returns the number of launches, their
 * summed duration and their summed ALGORITHMIC flops (2*M*K*Cout per launch). */
#define RCGAN_PROF_CONV_MFMA_128 1   /* conv_mfma_kernel<128,128> (fwd + dgrad) */
#define RCGAN_PROF_CONV_MFMA_64 2    /* conv_mfma_kernel<64,64> */
#define RCGAN_PROF_WGRAD_MFMA 3      /* conv_mfma_wgrad_kernel */
#define RCGAN_PROF_CONV_P8 4         /* conv_mfma_p8_kernel: 256 x 256 tile, 8 wavefronts (fwd + dgrad of the 256-channel layers) */
#define RCGAN_PROF_CONV_P8N 5        /* conv_mfma_p8n_kernel: 256 x 128 tile */
#define RCGAN_PROF_GATHER_F32 7      /* gemm_gather_kernel (conv_direct.hip): the fp32 path's gather GEMM on the fp32 matrix cores */
#define RCGAN_PROF_ALLREDUCE 6       /* every all-reduce group of comm.hip (eager launches only); "flops" = bytes exchanged per rank */
int rcgan_prof_begin(rcgan_ctx* ctx, int which);
int rcgan_prof_end(rcgan_ctx* ctx, int* launches, double* total_ms, double* total_flops);
/* Flops the kernels of the last rcgan_prof_begin .. rcgan_prof_end section EXECUTED: equal to the algorithmic count except for
 * the sub-pixel form of the upsample-3x3 convolutions (four 2x2 convolutions with summed filters: 4/9 of the multiply-adds). */
int rcgan_prof_executed_flops(rcgan_ctx* ctx, double* executed_flops);
/* How many launches of that section also applied the batch norm in front of the convolution to their staged input
 * (rcgan_conv2d_fwd_bn_residual on a halo-patch kernel): their time includes that work, their FLOP count does not. */
int rcgan_prof_bn_in_launches(rcgan_ctx* ctx, int* launches);
/* Diagnostics: while `stamps` is non-null, every workgroup of the 256 x 256 convolution kernel writes 8 x uint64 to
 * stamps[workgroup * 8 ..]: s_memtime at {start, tap table built, first K-tile landed, K loop done, stores issued,
 * stores complete}, HW_ID, XCC_ID (scripts/exp_p8_timeline.py).  Pass null to switch it off. */
int rcgan_debug_stamps(rcgan_ctx* ctx, void* stamps);
/* hipGraph capture of everything launched on the ctx stream between begin/end; replay with launch.
 * Replaces the per-step sess.run dispatch (gan_resnet.py:931,938; mnist/model.py:347-372). */
int rcgan_graph_begin(rcgan_ctx* ctx);
int rcgan_graph_end(rcgan_ctx* ctx, int* graph_id);
/* Capture contract of the entry points that take NO workspace argument.  The fp32 path of rcgan_conv2d_fwd, rcgan_deconv2d_bwd_data[_cols],
 * rcgan_linear_bwd_data and the narrow (<= 2 output channels) data gradient keep partial tiles / per-source-pixel products in two scratch
 * buffers hidden in the context that grow on demand with hipMalloc.  An allocation cannot be captured: inside rcgan_graph_begin .. end a call
 * that would have to grow a buffer returns RCGAN_EHIP (hipErrorStreamCaptureUnsupported) and the capture has to be dropped with
 * rcgan_graph_abort.  So before capturing either run every shape of the captured body once eagerly, or reserve the scratch up front:
 * rcgan_reserve_scratch grows BOTH buffers to at least `bytes` each (never inside a capture; buffers only grow; an outgrown buffer stays
 * alive until rcgan_destroy because earlier graphs address it).  Upper bounds: split reduction 8 x 4 bytes x the output elements of the
 * largest GEMM with < 128 output tiles of 64 x 64 (<= 16 MiB); narrow data gradient 4 bytes x n x oh x ow x kh x kw x cin of the layer.
 * rcgan_scratch_bytes reports the current sizes (either pointer may be null). */
int rcgan_reserve_scratch(rcgan_ctx* ctx, size_t bytes);
int rcgan_scratch_bytes(rcgan_ctx* ctx, size_t* split_reduction_bytes, size_t* narrow_bytes);
/* Leave a capture that a failed launch has made impossible to finish; what was recorded is dropped (nothing of it ran). */
int rcgan_graph_abort(rcgan_ctx* ctx);
int rcgan_graph_launch(rcgan_ctx* ctx, int graph_id);
int rcgan_graph_destroy(rcgan_ctx* ctx, int graph_id);

/* ---- convolution ---------------------------------------------------------------------------- */
#define RCGAN_CONV_IN_UPSAMPLE2X 1  /* conv reads nearest-2x-upsampled input (gan_resnet.py:263-264 folded in) */
#define RCGAN_CONV_IN_RELU 2        /* relu applied to the input on load (gan_resnet.py:305,317,347) */
#define RCGAN_CONV_ACCUMULATE 4     /* out += result (residual add, gan_resnet.py:328,353) */
#define RCGAN_CONV_FORCE_DIRECT 8   /* testing: bypass the MFMA path */
#define RCGAN_CONV_OUT_MEANPOOL2 16 /* ConvMeanPool (gan_resnet.py:241-247): the 2x2 mean pool folded into the convolution -- y [n,h/2,w/2,cout] =
                                      * meanpool2(conv(x)) + bias, computed as ONE 4x4 stride-2 convolution with summed filters (4/9 of the
                                      * multiply-adds), only where rcgan_conv_fused_pool_ok says so.  In rcgan_conv2d_bwd_weight[_group] the
                                      * flag means "dy is the POOLED gradient [n,h/2,w/2,cout]" (sub-pixel filter gradient, 4/9 of the
                                      * multiply-adds, no spread dy), only where rcgan_conv_wgrad_pool_ok says so */

#define RCGAN_CONV_RESID_UPSAMPLE2X 32 /* rcgan_conv2d_fwd_residual: the residual is [n,h/2,w/2,cout] and is added nearest-upsampled -- the
                                      * shortcut of an up block evaluated BEFORE the upsample (a 1x1 convolution commutes with it:
                                      * gan_resnet.py:258-272, 295-328), a quarter of its multiply-adds and of its bytes; only where
                                      * rcgan_conv_resid_up_ok says so */

typedef struct rcgan_conv_desc {
  int n, h, w, cin;   /* logical conv input: after the 2x upsample when IN_UPSAMPLE2X is set */
  int cout, kh, kw, stride;
  int dtype;          /* RCGAN_F32 or the build's 16-bit dtype (rcgan_half_dtype()): activations and activation gradients */
  int flags;
} rcgan_conv_desc;

/* Filter preparation: master fp32 HWIO filter (optionally divided by *sigma, the spectral norm) ->
 * the layouts the conv kernels consume.  `prepared` must hold rcgan_conv_prepared_bytes(desc).
 * Replaces the W_bar = W / sigma reshape (mnist/sn.py:55-62) + the filter argument of tf.nn.conv2d. */
size_t rcgan_conv_prepared_bytes(const rcgan_conv_desc* d);
int rcgan_conv_prepare(rcgan_ctx* ctx, const rcgan_conv_desc* d, const float* w_hwio,
                       const float* sigma /* device scalar or NULL */, void* prepared);

/* The same for many filters in ONE launch (every conv of a network at the start of a step).  items: HOST array. */
typedef struct rcgan_prepare_item {
  rcgan_conv_desc desc;      /* only kh, kw, cin, cout, stride, dtype, flags matter */
  const float* w;
  const float* sigma;        /* device scalar or NULL */
  void* prepared;            /* rcgan_conv_prepared_bytes(&desc) */
} rcgan_prepare_item;
int rcgan_conv_prepare_batch(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items);
/* The same launch with the projection head's label embeddings riding in it as extra workgroups:
 * E[l][j] = (sum_k table[l][k] * w_e[k][j]) / sigma_e + b_e[j]  (embedding.py:29-51 + D.Embedding_y, gan_resnet.py:414-421).
 * E depends on parameters only; computed here it leaves the step's dependency chain (rcgan_head_desc::E_pre).  e may be NULL.
 * v <= 16 (the rider's LDS); a model of more classes computes E inside rcgan_proj_head_fwd_bwd instead. */
typedef struct rcgan_embed_desc {
  int v, e_dim, d;
  const float *table, *w_e, *sigma_e /* device scalar or NULL */, *b_e /* or NULL */;
  float* E;               /* [v][d] */
} rcgan_embed_desc;
int rcgan_conv_prepare_batch_embed(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e);
/* ... and with the critic step's INPUT work riding too (it depends on the step's inputs, not on its parameters, and would otherwise
 * be five launches at the head of the step's dependency chain): dequantisation noise noise[i] ~ U[noise_lo, noise_hi) drawn from the
 * device stream exactly as rcgan_rng_fill(kind 0) over n*3072 floats would (the stream then advances by as much), the preprocessing
 * of rcgan_preprocess_cifar into rows [0, n) of x [2n,32,32,3] (gan_resnet.py:548-551), the 2x2 mean pool of all 2n images
 * (rows [n, 2n) = the fakes: already in x, or copied there from a slice of `fakes`; pooled [2n,16,16,3] or NULL: D.Block.1's shortcut input, :239-240, :346) and a
 * zero-fill of fill_count floats (the gradient slab; or NULL).  Same bits as the separate entry points.  e / si may be NULL. */
typedef struct rcgan_step_inputs_desc {
  int n, dtype;
  const int32_t* images;   /* [n][3][32][32] */
  void* x; void* pooled;
  float noise_lo, noise_hi;
  uint64_t seed; void* rng_state;
  float* fill; size_t fill_count;
  /* optional: the step's fakes are slice *fake_slice (a device counter, moved on mod n_slices by the launch) of
   * fakes [n_slices][n][32][32][3]: copied into rows [n, 2n) of x by the same launch.  NULL: they are in x already. */
  const void* fakes; void* fake_slice; int n_slices;
} rcgan_step_inputs_desc;
int rcgan_conv_prepare_batch_riders(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e,
                                    const rcgan_step_inputs_desc* si);
/* (round 6) ... and the fragment-major filter copies the fused 8x8 stage and the register-filter kernel read (rcgan_dtrunk*,
 * rcgan_conv2d_rf; the layout of rcgan_fragments_prepare), written by the SAME launch straight from the fp32 weights instead of by a
 * launch of its own behind it: frags[i] names items[frags[i].item] (a 16-bit 3x3 stride-1 filter, channels % 64 == 0) and the two
 * destinations -- forward rows / rotated data-gradient rows, 9*cin*cout elements each -- with ctn channel tiles of 16 rows per block and
 * ss K-steps of 32 per slice (the 8x8 stage: 2, 36; the register-filter kernel: 4, 18).  Bit-identical to rcgan_conv_prepare +
 * rcgan_fragments_prepare (the same fp32 product W / sigma rounded once).  At most 12 per call; e / si may be NULL. */
typedef struct rcgan_frag_item { int item; int ctn, ss; void* fwd; void* bwd; } rcgan_frag_item;
int rcgan_conv_prepare_batch_frags(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e,
                                   const rcgan_step_inputs_desc* si, const rcgan_frag_item* frags, int n_frags);

size_t rcgan_conv_workspace_bytes(const rcgan_conv_desc* d);
/* y = conv2d_SAME(x, w) (+bias).  Replaces tf.nn.conv2d + bias_add: mnist/ops.py:62-65,
 * cifar10/common/ops/conv2d.py:181-216.  x: [n, h(/2), w(/2), cin]; y: [n, oh, ow, cout]. */
/* 1 if the matrix-core kernels take d (3x3, stride 1, 16-bit, power-of-two image, channels % 64 == 0) with RCGAN_CONV_OUT_MEANPOOL2 */
int rcgan_conv_fused_pool_ok(const rcgan_conv_desc* d);
/* 1 if rcgan_conv2d_fwd_residual takes d with RCGAN_CONV_RESID_UPSAMPLE2X */
int rcgan_conv_resid_up_ok(const rcgan_conv_desc* d);
int rcgan_conv2d_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared,
                     const float* bias /* or NULL */, void* y);
/* y = conv2d_SAME(x, w) (+bias) + residual: the pre-activation residual sum `shortcut + output` of
 * gan_resnet.py:328 folded into the convolution's epilogue.  residual: [n, oh, ow, cout] or NULL, must not alias y. */
/* y = conv2d_SAME(act(batch_norm(x))) (+bias) with the (conditional) batch norm + activation of cond_batchnorm / nonlinearity
 * (normalization.py:27-59, gan_resnet.py:350-352) applied to the convolution's staged input instead of being written out and read back:
 * for a forward-only pass (the critic steps' generator forwards) the normalised tensor never exists.  x: the batch norm's INPUT;
 * mean / rstd [segments][cin] from rcgan_bn_fwd_segments(..., y = NULL) (statistics only) or rcgan_bn_stats; gamma / beta [n_labels][cin];
 * labels [n] or NULL (any n_labels up to 1024: each workgroup stages only its image's [2][cin] affine).  Same values as rcgan_bn_apply_* followed by rcgan_conv2d_fwd (the affine is evaluated in the same fp32
 * sequence and rounded to 16 bits at the same point).  rcgan_conv_bn_in_ok: the small-output image-end layers (G.Output: 256 -> 3) and
 * (round 5) the 3x3 / upsample-3x3 layers the halo-patch kernels take (conv_mfma8h.hip: 16- / 32-wide (low-resolution) images, enough
 * 256-pixel tiles to fill the chip -- G.Block.2.Conv2, G.Block.3.Conv1 / Conv2 at the bench batches); d->flags may carry
 * RCGAN_CONV_IN_UPSAMPLE2X (the norm sits in front of the upsample, as in UpsampleConv) and, for the _residual form,
 * RCGAN_CONV_RESID_UPSAMPLE2X; not IN_RELU (the norm's own activation is `act`: RCGAN_ACT_NONE or RCGAN_ACT_RELU), ACCUMULATE, OUT_MEANPOOL2. */
int rcgan_conv_bn_in_ok(const rcgan_conv_desc* d);
int rcgan_conv2d_fwd_bn(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, void* y,
                        int segments, const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        int act);
/* ... + residual in the epilogue (rcgan_conv2d_fwd_residual's forms; halo-patch kernels only when residual != NULL). */
int rcgan_conv2d_fwd_bn_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias,
                                 const void* residual, void* y, int segments, const int32_t* labels, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, int act);
int rcgan_conv2d_fwd_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared,
                              const float* bias /* or NULL */, const void* residual /* or NULL */, void* y);
/* dx = d(conv)/dx.  With IN_RELU, dx is masked by x>0 (x = the pre-activation input).  With
 * IN_UPSAMPLE2X dx is the gradient w.r.t. the low-resolution input.  ACCUMULATE: dx += ...
 * Replaces tf.nn.conv2d_backprop_input (autodiff of the above).  ws: rcgan_conv_workspace_bytes. */
int rcgan_conv2d_bwd_data(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* prepared,
                          const void* x /* needed with IN_RELU */, void* dx, void* ws, size_t ws_bytes);
/* dx = conv2d_backprop_input(dy) (masked by x > 0 under RCGAN_CONV_IN_RELU) + residual, written out of place: the
 * accumulate of a second gradient contribution without touching the buffer that holds the first one (needed when that
 * buffer is still to be read, e.g. by a deferred filter gradient).  residual: [n, h, w, cin], must not alias dx.
 * ws: rcgan_conv_workspace_bytes(d), as for rcgan_conv2d_bwd_data. */
int rcgan_conv2d_bwd_data_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* prepared,
                                   const void* x /* IN_RELU mask or NULL */, const void* residual, void* dx, void* ws, size_t ws_bytes);
/* dw (fp32 HWIO) = d(conv)/dw (dw = or += by accumulate), dbias = sum dy (if non-NULL).
 * Replaces tf.nn.conv2d_backprop_filter + BiasAddGrad.  Upsample-3x3 (IN_UPSAMPLE2X: x stored at [n,h/2,w/2,cin]) and
 * ConvMeanPool (OUT_MEANPOOL2: dy pooled) layers on the matrix cores are computed in their sub-pixel form: 16 Cin x Cout
 * products over the low-resolution grid folded into the 9 taps by the slab reduction, instead of 9 over the full one.
 * ws: rcgan_conv_workspace_bytes(d). */
/* 1 if rcgan_conv2d_bwd_weight takes d with RCGAN_CONV_OUT_MEANPOOL2 (dy = the pooled gradient) */
int rcgan_conv_wgrad_pool_ok(const rcgan_conv_desc* d);
int rcgan_conv2d_bwd_weight(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy,
                            float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes);
/* The filter gradients of `n` layers in one call (all x / dy available: the end of a backward pass).  Same results as n
 * rcgan_conv2d_bwd_weight calls; the layers the three-tap matrix-core kernel takes share ONE launch (+ one slab reduction):
 * the discriminator's 8x8 / 16x16 layers are launch-latency-bound one by one.  dbiases[i] may be NULL.
 * ws: rcgan_conv2d_bwd_weight_group_workspace_bytes(n, descs) suffices.  The call splits ws in two halves: the first holds the slabs of
 * the grouped launches, the second serves every layer computed by a call of its own -- a layer whose slabs do not fit the first half is
 * one of those (same values), so any ws of at least twice the largest rcgan_conv_workspace_bytes of the layers is enough to be correct.
 * The call plans all its launches before the first of them: a failure while planning (a bad descriptor, a shape no kernel takes) returns
 * with nothing of this call launched. */
size_t rcgan_conv2d_bwd_weight_group_workspace_bytes(int n, const rcgan_conv_desc* descs);
int rcgan_conv2d_bwd_weight_group(rcgan_ctx* ctx, int n, const rcgan_conv_desc* descs, const void* const* xs, const void* const* dys,
                                  float* const* dws, float* const* dbiases, int accumulate, void* ws, size_t ws_bytes);

/* Transposed convolution, filter [kh][kw][Cout][Cin] used as-is (no preparation, fp32).
 * d describes the *forward conv* it is the gradient of: n,h,w,cin = deconv OUTPUT (n,H,W,Cout_deconv),
 * d.cout = deconv input channels.  Replaces tf.nn.conv2d_transpose at mnist/ops.py:78-79. */
int rcgan_deconv2d_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const float* w,
                       const float* bias, void* y);
int rcgan_deconv2d_bwd_data(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const float* w, void* dx);
/* ... only the first n_cols input channels of it, dense ([n, h', w', n_cols]; RCGAN_CONV_ACCUMULATE in d.flags adds onto dx): the input of
 * the generator's transposed convolutions is conv_cond_concat(x, y) (mnist/ops.py:46-51, model.py:716-726) and the label channels need no
 * gradient -- the x part lands straight in x's gradient, a third of the column tiles (138 -> 128 channels) and the split kernel go away.
 * n_cols = 0: all of them. */
int rcgan_deconv2d_bwd_data_cols(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const float* w, void* dx, int n_cols);
/* dw [kh][kw][Cout][Cin] (= or +=), dbias = sum dy.  ws: rcgan_conv_workspace_bytes(d). */
int rcgan_deconv2d_bwd_weight(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy,
                              float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes);
/* The same filter gradient for x = conv_cond_concat(t, yb) (mnist/ops.py:46-51; the generator's g_h2 / g_h3, model.py:722-731): the first
 * n_cols channels of x are real, the other d.cout - n_cols (<= 16) are yb[n][:] (fp32 [n][d.cout - n_cols]) on every pixel.  The gather
 * GEMM runs over the n_cols real columns only (for 128 + 10 channels: two 64-wide column tiles instead of three); the label columns are
 * dW[kh][kw][c][n_cols + l] = sum_n yb[n][l] * (sum of dy[n] over the sub-grid of output pixels tap (kh, kw) reaches): one pass over dy, a
 * small product, and one reduction that writes all d.cout columns.  Same values as rcgan_deconv2d_bwd_weight up to fp32 summation
 * order.  Workspace: rcgan_deconv2d_bwd_weight_concat_bytes(d, n_cols). */
size_t rcgan_deconv2d_bwd_weight_concat_bytes(const rcgan_conv_desc* d, int n_cols);
int rcgan_deconv2d_bwd_weight_concat(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, int n_cols, const float* yb,
                                     float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes);

/* ---- dense ----------------------------------------------------------------------------------- */
/* y[m,n] = x[m,k] @ w[k,n] (+bias).  w fp32 row-major, optionally divided by *sigma.
 * Replaces tf.matmul + bias: mnist/ops.py:114-116, cifar10/common/ops/linear.py:161-180. */
int rcgan_linear_fwd(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* x, const float* w,
                     const float* sigma, const float* bias, void* y);
int rcgan_linear_bwd_data(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* dy, const float* w,
                          const float* sigma, void* dx, int accumulate);
/* dw is the gradient w.r.t. the matrix actually multiplied (W or W_bar).  ws: rcgan_linear_workspace_bytes(m, k, n). */
int rcgan_linear_bwd_weight(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* x, const void* dy,
                            float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes);
size_t rcgan_linear_workspace_bytes(int m, int k, int n);

/* ---- normalisation ----------------------------------------------------------------------------- */
/* Batch statistics over rows of x[rows][c]: mean, biased var -> rstd = rsqrt(var+eps).
 * moving_mean / moving_var (may be NULL) get the TF fused-batch-norm update
 * m -= (m - batch)*(1-decay) with the UNBIASED variance (mnist/ops.py:38-44).
 * ws: rcgan_bn_workspace_bytes(rows, c) for up to 16 labels; rcgan_bn_workspace_bytes_labels(rows, c, n_labels) grows with the
 * label count (the per-label tables of the non-power-of-two apply paths) and equals the former for n_labels <= 16.
 * Label bounds of the conditional calls below: 1 <= n_labels <= 1024, every label in [0, n_labels). */
size_t rcgan_bn_workspace_bytes(int rows, int c);
size_t rcgan_bn_workspace_bytes_labels(int rows, int c, int n_labels);
int rcgan_bn_stats(rcgan_ctx* ctx, int rows, int c, int dtype, const void* x, float eps,
                   float* mean, float* rstd, float* moving_mean, float* moving_var, float decay,
                   void* ws, size_t ws_bytes);
/* y = act( gamma[l]*(x-mean)*rstd + beta[l] ), l = labels[row / rows_per_sample] (labels NULL -> row 0
 * of a [1][c] table = plain batch norm).  Replaces tf.nn.batch_normalization + embedding_lookup
 * (cifar10/common/ops/normalization.py:47-57) and tf.contrib.layers.batch_norm (mnist/ops.py:38-44)
 * fused with the following relu / lrelu (gan_resnet.py:305,317,366; mnist/model.py:661-719).
 * Every batch-norm call returns RCGAN_EINVALID_ARG, before it launches anything, for a non-positive shape, n_labels outside
 * 1 .. 1024, n_labels > 1 with labels NULL (rcgan_bn_fwd_segments with y = NULL included), or a NULL tensor it would touch.
 * ws: rcgan_bn_workspace_bytes_labels(n*rows_per_sample, c, n_labels). */
int rcgan_bn_apply_fwd(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype, const void* x,
                       const int32_t* labels, const float* gamma, const float* beta,
                       const float* mean, const float* rstd, int act, void* y, void* ws, size_t ws_bytes);
/* rcgan_bn_stats + rcgan_bn_apply_fwd for `nseg` independent segments of n_per_seg samples stored back to back: each
 * segment is normalised with its OWN batch statistics (= nseg separate Generator() calls of the reference, e.g. the
 * N_CRITIC generator forwards of one iteration, gan_resnet.py:540-546,928-947, evaluated as one batch).  Forward only.
 * mean / rstd: [nseg][c] outputs; ws: nseg * rcgan_bn_workspace_bytes(n_per_seg*rows_per_sample, c). */
int rcgan_bn_fwd_segments(rcgan_ctx* ctx, int nseg, int n_per_seg, int rows_per_sample, int c, int n_labels, int dtype,
                          const void* x, const int32_t* labels, const float* gamma, const float* beta, float eps, int act,
                          float* mean, float* rstd, void* y, void* ws, size_t ws_bytes);
/* Backward of stats+apply (gradient flows through the batch statistics).  dgamma/dbeta: [n_labels][c]
 * (= or += by accumulate); dx = or += by accumulate_dx.  y is the forward output (activation mask).
 * n_labels <= 16: per-label accumulators in registers / LDS (the fused, tree and generic paths).  17 .. 1024: per-sample partials
 * in ws, then a deterministic fp64 reduction per (label, channel) in sample order; a label absent from the batch gets 0 (left
 * untouched under accumulate).  ws: rcgan_bn_workspace_bytes_labels(n*rows_per_sample, c, n_labels).  With labels EVERY route keeps at
 * least one partial row [2*c] per sample.  In floats: (n + 1)*2*c on the scalar and the power-of-two-c routes, (n + 2)*2*c on the
 * per-sample route (n_labels > 16), (n + 2)*2*c + n_labels*c where the c % 8 == 0 route holds its tables.  The query returns at least
 * 8210*2*c + 64 floats (exactly that while n*rows_per_sample <= 4094*512; + 2*(n_labels - 16)*c past 16 labels), which covers every
 * n <= 8192.  Past it, with exactly the query's bytes, at the earliest: the c % 8 == 0 route no longer holds its tables, and the call
 * takes the scalar kernels, from the first n > 8208 - n_labels/2 + 32/c (16 labels, c >= 40: 8201); the call returns
 * RCGAN_EWORKSPACE_TOO_SMALL before it launches anything from n = 8210 + floor(32/c) for n_labels <= 16 (c >= 33: 8210, c = 17 .. 32:
 * 8211) and from n = 8209 + (n_labels - 16) + floor(32/c) for n_labels > 16, and its message names the bytes it needs
 * (tests/tools/bn_plan_sweep.cpp finds these n for channel counts on either side of each step). */
int rcgan_bn_bwd(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype,
                 const void* x, const void* y, const void* dy, const int32_t* labels,
                 const float* gamma, const float* mean, const float* rstd, int act,
                 void* dx, int accumulate_dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes);
/* rcgan_bn_bwd with the forward's beta (offset) table: for ReLU / leaky-ReLU the activation mask is then recomputed from x with
 * the forward's exact arithmetic (the fused power-of-two-channel kernels), so y is not read: 2 instead of 3 tensor reads per pass.
 * ws: rcgan_bn_workspace_bytes_labels(n*rows_per_sample, c, n_labels), as rcgan_bn_bwd. */
int rcgan_bn_bwd2(rcgan_ctx* ctx, int n, int rows_per_sample, int c, int n_labels, int dtype, const void* x, const void* y,
                  const void* dy, const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd,
                  int act, void* dx, int accumulate_dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes);
/* Inference-mode batch norm with moving statistics (gen_sampler, mnist/model.py:745-754). */
int rcgan_bn_infer(rcgan_ctx* ctx, int rows, int c, int dtype, const void* x, const float* gamma,
                   const float* beta, const float* moving_mean, const float* moving_var, float eps,
                   int act, void* y);
/* Its adjoint w.r.t. x: dx (= or +=) dy * act'(y) * gamma / sqrt(moving_var + eps).  Used by recover_labels
 * (mnist/model.py:494-640), which differentiates the frozen sampler w.r.t. its latent input.  act' is taken from the OUTPUT y for
 * every activation (ReLU / leaky ReLU: its sign, y = 0 counting as the negative side); y may be NULL for RCGAN_ACT_NONE.
 * Both calls return RCGAN_EINVALID_ARG, before they launch anything, for a non-positive shape or a NULL tensor they would touch. */
int rcgan_bn_infer_bwd(rcgan_ctx* ctx, int rows, int c, int dtype, const void* y, const void* dy, const float* gamma,
                       const float* moving_var, float eps, int act, void* dx, int accumulate);

/* ---- spectral normalisation (mnist/sn.py:31-75 == cifar10/common/ops/sn.py:31-75) --------------- */
typedef struct rcgan_sn_item {
  const float* w;   /* [k][c] (any filter reshaped to [-1, c]) */
  float* u;         /* [c] persistent; overwritten with u' iff update != 0 */
  float* sigma;     /* [1] out */
  float* save;      /* scratch kept for the backward: rcgan_sn_save_floats(k,c) floats */
  int k, c, update;
} rcgan_sn_item;
size_t rcgan_sn_save_floats(int k, int c);
/* One power iteration for every item in one launch (items: HOST array, copied into the launch). */
int rcgan_sn_power_iter(rcgan_ctx* ctx, const rcgan_sn_item* items, int n_items);
typedef struct rcgan_sn_bwd_item {
  const float* w; const float* dwbar; float* dw; float* save /* also scratch */; int k, c, accumulate;
} rcgan_sn_bwd_item;
/* dW from dW_bar, differentiating THROUGH the power iteration (no stop_gradient in the reference). */
int rcgan_sn_bwd(rcgan_ctx* ctx, const rcgan_sn_bwd_item* items, int n_items);
/* The same two launches with the optimiser of a SINGLE-RANK step in the second (round 6): after dW is formed for a chunk of
 * rows, TF ApplyAdam (tf.train.AdamOptimizer, gan_resnet.py:802-808; the arithmetic of rcgan_adam_tf) updates those rows of the
 * optimiser group's slabs w / m / v in place; rider workgroups do the same for the slab's other parameters (`ranges`: host array
 * of n_ranges {lo, hi} float offsets, at most 48).  Items and ranges must tile [0, count) exactly, every item's w / dw must point into
 * w / g at the same offset, count < 2^32.  An item with c % 4 == 0 takes the float4 path: its slab offset must be a multiple of 4 floats,
 * and its w, dwbar, dw, save as well as the slabs m and v must be 16-byte aligned (RCGAN_EINVALID_ARG otherwise).  hyper: DEVICE
 * {lr, t} with t = the number of updates applied so far: the call advances it by one (in its first launch) and uses the advanced
 * value for the bias correction -- a captured step replays with a fresh count, the host rewrites the pair only when lr changes.
 * dW is still written to g.  Not for data-parallel steps (the all-reduce sits between the gradient and the update) nor for a
 * dynamic loss scale (the overflow verdict does). */
typedef struct rcgan_sn_adam {
  float* w; float* g; float* m; float* v; size_t count;
  float* hyper;
  float beta1, beta2, eps, clip, grad_scale;
  int n_ranges; const size_t* ranges;
} rcgan_sn_adam;
int rcgan_sn_bwd_adam(rcgan_ctx* ctx, const rcgan_sn_bwd_item* items, int n_items, const rcgan_sn_adam* opt);

/* ---- elementwise / resampling -------------------------------------------------------------------- */
int rcgan_act_fwd(rcgan_ctx* ctx, size_t count, int dtype, int act, const void* x, void* y);
/* dx = dy * act'(.)  (mask/derivative taken from y for tanh/sigmoid, from x for relu/lrelu). */
int rcgan_act_bwd(rcgan_ctx* ctx, size_t count, int dtype, int act, const void* x_or_y, const void* dy,
                  void* dx, int accumulate);
int rcgan_add(rcgan_ctx* ctx, size_t count, int dtype, const void* a, const void* b, void* y);
int rcgan_axpby(rcgan_ctx* ctx, size_t count, int dtype, float alpha, const void* a, float beta, void* y);
int rcgan_cast(rcgan_ctx* ctx, size_t count, int src_dtype, const void* src, int dst_dtype, void* dst);
/* 2x2 mean pool (gan_resnet.py:239-240) and its adjoint; nearest 2x upsample (:263-264) and its adjoint. */
int rcgan_meanpool2_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y);
int rcgan_meanpool2_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* dy, void* dx, int accumulate);
int rcgan_upsample2_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y);
int rcgan_upsample2_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* dy, void* dx, int accumulate);
/* y[n,h,w,:c1] = x ; y[n,h,w,c1:] = onehot rows yb[n,:c2]  (conv_cond_concat, mnist/ops.py:46-51);
 * the adjoint copies the first c1 channels back. */
/* Zero-pad the channel axis: y[rows][before + c + after] (tf.pad; the option-A shortcut of the generated-label-accuracy
   classifier, cifar10/resnet-110/graph_optimized.pb used by gan_resnet.py:424-455).  Inference only. */
int rcgan_pad_channels(rcgan_ctx* ctx, size_t rows, int c, int before, int after, int dtype, const void* x, void* y);
int rcgan_concat_channels_fwd(rcgan_ctx* ctx, int n, int hw, int c1, int c2, int dtype, const void* x,
                              const float* yb, void* y);
int rcgan_concat_channels_bwd(rcgan_ctx* ctx, int n, int hw, int c1, int c2, int dtype, const void* dy, void* dx);
/* The batch repeated `reps` times back to back, y[r][i] = x[i] (count elements per copy), and its adjoint dx[i] (+)= sum_r dy[r][i]:
 * the reference's ten discriminator() calls on the same images, one per label (mnist/model.py:152-163 `unbiased`, :187-197
 * `estimate_confuse`), as ONE pass over 10 x batch samples for the discriminators whose convolutions see the label
 * (disc_type=vanilla, --concat_y).  rcgan_transpose_f32: y[c][r] (+)= x[r][c] -- that pass's [labels][samples] logits as the
 * [samples][labels] matrix of tf.concat(D_logits_all, 1) (:165,199), and the adjoint. */
int rcgan_tile_rows_fwd(rcgan_ctx* ctx, size_t count, int reps, int dtype, const void* x, void* y);
int rcgan_tile_rows_bwd(rcgan_ctx* ctx, size_t count, int reps, int dtype, const void* dy, void* dx, int accumulate);
int rcgan_transpose_f32(rcgan_ctx* ctx, int rows, int cols, const float* x, float* y, int accumulate);
/* uint8-as-int32 CHW [n][3][32][32] + dequantisation noise (fp32, CHW order) -> NHWC in [-1,1):
 * 2*(x/256-.5)+noise (gan_resnet.py:548-551). */
int rcgan_preprocess_cifar(rcgan_ctx* ctx, int n, const int32_t* images_chw, const float* noise_chw,
                           int dtype, void* y_nhwc);

/* Counter-based device RNG (Philox4x32-10).  kind 0: uniform [lo,hi); kind 1: normal(mean=lo, std=hi).
 * Quad q of a stream is philox4x32-10 of the counter {lo32(offset + q), hi32(offset + q), 0x5eed5eed, 0} under the key
 * {lo32(seed), hi32(seed)}; a draw of count numbers takes ceil(count / 4) quads (the last one may be cut).  With u = (r >> 8) * 2^-24
 * of a word r, kind 0 is the fp32 number lo + (hi - lo) * u, and kind 1 is Box-Muller on the word pairs (0, 1) and (2, 3) of a quad
 * with u = ((float)(r >> 8) + 0.5f) * 2^-24.  Kind 0 needs finite lo < hi and returns values of the OUTPUT type in [lo, hi): the fp32
 * number is kept at the largest float below hi (the sum can round up to hi when lo != 0), and a 16-bit result between the smallest
 * 16-bit value >= lo and the largest one < hi (EINVALID_ARG when there is none); fp32 draws with lo = 0 are hi * u unchanged.
 * state: DEVICE uint64[1] stream offset, advanced on the stream after the draw (so a replayed graph
 * draws fresh numbers), or NULL for offset 0.  Replaces tf.random_normal (gan_resnet.py:359) and the
 * tf.random_uniform dequantisation noise (gan_resnet.py:549); the TF Philox stream itself is not
 * reproducible, parity tests feed explicit noise instead. */
int rcgan_rng_fill(rcgan_ctx* ctx, size_t count, int dtype, int kind, float lo, float hi, uint64_t seed,
                   void* state, void* y);

/* ---- discriminator head + losses -------------------------------------------------------------------- */
/* Every entry point of this section returns RCGAN_EINVALID_ARG, before it launches anything, for a non-positive dimension or a
 * NULL tensor it would read or write (the optional ones are named at each call). */
/* feat[n][c] = mean_hw(relu(x)) (gan_resnet.py:405-407; act = RCGAN_ACT_NONE gives the plain spatial
 * mean of mnist/model.py:679) and its adjoint. */
int rcgan_act_meanhw_fwd(rcgan_ctx* ctx, int n, int hw, int c, int dtype, int act, const void* x, float* feat);
int rcgan_act_meanhw_bwd(rcgan_ctx* ctx, int n, int hw, int c, int dtype, int act, const void* x,
                         const float* dfeat, void* dx);
/* rows gathered from a [v][d] table / scatter-added back (tf.nn.embedding_lookup, embedding.py:51).  No bound on v (idx in [0, v)). */
int rcgan_gather_rows(rcgan_ctx* ctx, int n, int d, const float* table, const int32_t* idx, float* out);
int rcgan_scatter_add_rows(rcgan_ctx* ctx, int n, int d, int v, const float* src, const int32_t* idx,
                           float* table_grad, int accumulate);
/* logit[n] = psi[n] + <feat[n,:], emb[n,:]>  (gan_resnet.py:588,763; mnist/model.py:685) + adjoint.  psi may be NULL (no offset).
 * Adjoint: dfeat (= or += by acc_feat) dlogit * emb, dpsi = dlogit, demb = dlogit * feat; each of the three may be NULL (skipped);
 * emb is read only for dfeat, feat only for demb. */
int rcgan_proj_logit_fwd(rcgan_ctx* ctx, int n, int d, const float* feat, const float* psi, const float* emb,
                         float* logit);
int rcgan_proj_logit_bwd(rcgan_ctx* ctx, int n, int d, const float* feat, const float* emb, const float* dlogit,
                         float* dfeat, float* dpsi, float* demb, int acc_feat);
/* logits[n][v] = psi[n] + <feat[n,:], E[v,:]> for every label v (rcgan-u: gan_resnet.py:654-660, 737-740;
 * the reference re-runs the projection for all 10 labels -- features are computed once here) + adjoint.  No bound on v: a wavefront
 * per logit, a thread per output of the adjoint (v <= 1024 in the models).  psi and all three outputs of the adjoint (dfeat = or += by
 * acc_feat; dpsi, dE written) are required. */
int rcgan_proj_logit_all_fwd(rcgan_ctx* ctx, int n, int d, int v, const float* feat, const float* psi,
                             const float* E, float* logits);
int rcgan_proj_logit_all_bwd(rcgan_ctx* ctx, int n, int d, int v, const float* feat, const float* E,
                             const float* dlogits, float* dfeat, float* dpsi, float* dE, int acc_feat);
/* Loss terms.  Each adds weight*L to *loss_acc (device scalar) and WRITES dlogit = weight * dL/dlogit.
 *   kind HINGE_REAL: mean relu(1-x)   HINGE_FAKE: mean relu(1+x)   NEG_MEAN: -mean x  (gan_resnet.py:604-605,773)
 *   CE_ONES / CE_ZEROS: mean sigmoid_ce(x, 1|0) (mnist/model.py:139-145).  Their gradients are evaluated as -1 / (1 + e^x) (in the form
 *   -e^-x / (1 + e^-x) for x > 0, which shares the forward value's exponential) and 1 / (1 + e^-x), never as sigmoid(x) - 1: they keep their relative precision for saturated logits (as do those of
 *   rcgan_bce_onehot_fwd_bwd and rcgan_proj_head_fwd_bwd, which share the term)
 * x: [rows][cols]; optional row weights wts[rows][cols] turn the inner mean into
 * mean_rows( sum_cols( term * wts ) )  (unbiased :647, rcgan-u :684,759; mnist/model.py:201-204);
 * dwts (may be NULL) receives weight * dL/dwts (needed for the learned confusion matrix); wts, loss_acc and dlogit may be NULL too
 * (no weights; no value; evaluation).  One workgroup: any rows x cols
 * (the [B, K] weight rows of the K-class models included). */
#define RCGAN_LOSS_HINGE_REAL 0
#define RCGAN_LOSS_HINGE_FAKE 1
#define RCGAN_LOSS_NEG_MEAN 2
#define RCGAN_LOSS_CE_ONES 3
#define RCGAN_LOSS_CE_ZEROS 4
int rcgan_loss_fwd_bwd(rcgan_ctx* ctx, int kind, int rows, int cols, const float* x, const float* wts,
                       float weight, float* loss_acc, float* dlogit, float* dwts);
/* weight * mean over all rows*cols of sigmoid_cross_entropy_with_logits(x, onehot(labels))
 * (perm regulariser: gan_resnet.py:693-694,782-783; mnist/model.py:218-221). */
/* The 8x8 stage of the CIFAR discriminator -- D.Block.3 .. D.Block.6, four identity-shortcut residual blocks of two 3x3
 * convolutions 128 -> 128 each (gan_resnet.py:275-328, 398-404) -- as ONE launch: a workgroup carries one image through all
 * eight layers with the activations in LDS.  16-bit activations only; x0 / outs / masks are [n][8][8][128].
 *   forward  (backward = 0): layer 2b = h_b = conv1(relu(x_b)) + bias, layer 2b+1 = x_{b+1} = x_b + conv2(relu(h_b)) + bias;
 *            outs[i] receives layer i's output (outs[7] is the stage's output, the others are what the backward pass needs).
 *   backward (backward = 1): x0 = gradient of the stage's output; layers run last to first: masks[0] belongs to
 *            block 6's conv2 (mask = h_6), masks[1] to its conv1 (mask = x_6), ...; outs[2j] = dh (gradient at
 *            conv1's output), outs[2j+1] = dx (gradient at the block's input; outs[7] is the gradient of the stage's input).
 * rcgan_dtrunk_prepare: prepared[i] = rcgan_conv_prepare layout of layer i's 3x3 128 -> 128 filter in FORWARD order (forward rows,
 * then data-gradient rows) -> frag (rcgan_dtrunk_fragment_bytes()): both directions' filters re-laid fragment-major -- the 16 bytes a
 * lane feeds one MFMA with are contiguous per wavefront and K-step, so the stage's filter loads are whole KiB blocks; one launch per
 * set of weights, shared by the forward and the backward pass. */
size_t rcgan_dtrunk_fragment_bytes(void);
int rcgan_dtrunk_prepare(rcgan_ctx* ctx, const void* const* prepared, void* frag);
int rcgan_dtrunk(rcgan_ctx* ctx, int n, int backward, const void* x0, const void* frag, const float* const* bias,
                 const void* const* masks, void* const* outs);
/* The same stage with the discriminator's relu + mean over the 8 x 8 pixels (gan_resnet.py:405-407) at its boundary.  Forward: feat
 * (optional) receives the pooled features [n][128] fp32 of the stored 16-bit output.  Backward: with feat = the gradient of the pooled
 * features and xlast = outs[7] of the forward call, the incoming gradient dy[p][c] = xlast[p][c] > 0 ? feat[c] / 64 : 0 is formed
 * inside the launch and written to dy_out [n][8][8][128] for the last layer's filter gradient (x0 may be NULL).  The projection head
 * then runs on [n][128] features without touching the activations. */
int rcgan_dtrunk_pooled(rcgan_ctx* ctx, int n, int backward, const void* x0, const void* frag, const float* const* bias,
                        const void* const* masks, void* const* outs, float* feat, const void* xlast, void* dy_out);

/* ---- register-filter convolution (csrc/conv_rf.hip) -----------------------------------------------------------------------------
 * One 3x3 stride-1 SAME layer on a small image grid (8x8, 16x16; 128 -> 128 channels), forward or data gradient, with the workgroup's
 * filter slice in registers and its input patch resident in LDS: the same values as rcgan_conv2d_fwd(_residual) / rcgan_conv2d_bwd_data
 * up to fp32 summation order (tf.nn.conv2d + bias_add, conv2d_backprop_input: cifar10/common/ops/conv2d.py:181-216 for D.Block.2.Conv1).
 * rcgan_conv_rf_ok: 1 if the kernel takes d (flags within IN_RELU | ACCUMULATE).  rcgan_conv_rf_prepare: ONE launch re-lays n prepared
 * filters (rcgan_conv_prepare layout) fragment-major into frags[i] (rcgan_conv_rf_fragment_bytes each; both directions).
 * rcgan_conv2d_rf: backward = 0: y = conv(x) (+bias) (+residual), input ReLU under IN_RELU; backward = 1: x = dy, y = dx, masked by
 * mask_x > 0 under IN_RELU, += under ACCUMULATE, + residual. */
int rcgan_conv_rf_ok(const rcgan_conv_desc* d);
size_t rcgan_conv_rf_fragment_bytes(const rcgan_conv_desc* d);
int rcgan_conv_rf_prepare(rcgan_ctx* ctx, int n, const rcgan_conv_desc* descs, const void* const* prepared, void* const* frags);
/* rcgan_dtrunk_prepare (trunk_prepared = the stage's eight prepared filters in forward order, or NULL) and rcgan_conv_rf_prepare (n <= 12)
 * as ONE launch: every fragment-major copy a critic step needs. */
int rcgan_fragments_prepare(rcgan_ctx* ctx, const void* const* trunk_prepared, void* trunk_frag, int n, const rcgan_conv_desc* descs,
                            const void* const* prepared, void* const* frags);
int rcgan_conv2d_rf(rcgan_ctx* ctx, const rcgan_conv_desc* d, int backward, const void* x, const void* frag, const float* bias,
                    const void* mask_x, const void* residual, void* y);

/* ---- the 16x16 down block's forward as one launch (csrc/conv_dblock2.hip) ----------------------------------------------------------
 * D.Block.2 of the CIFAR critic (gan_resnet.py:275-328 with resample='down'), 16 x 16 x 128 -> 8 x 8 x 128, two workgroups per image:
 *   h = Conv1(relu(x)) + b1;  xp = meanpool2(x);  t = Shortcut(xp) + bs;  y = t + meanpool2(Conv2(relu(h)) + b2)
 * with the 16-bit rounding points of the four launches it replaces (h, xp, t, y): h and xp are bit-identical to rcgan_conv2d_rf and
 * rcgan_meanpool2_fwd, and Conv2's reduction runs in the order of the gather-form tile kernel with two K-split groups (the kernel the
 * training step's shape takes), so y has the four launches' bits there and differs by fp32 summation order at most elsewhere.  h, xp and y are what the block's (unfused) backward pass reads.
 * rcgan_dblock2_ok: 1 if d is Conv1's descriptor of exactly that block (3x3, stride 1, RCGAN_CONV_IN_RELU alone, the build's 16-bit
 * dtype, any n >= 1) and both fragment copies exist.  conv1_frag: Conv1's copy of rcgan_conv_rf_prepare / rcgan_fragments_prepare;
 * dblock2_frag (rcgan_dblock2_fragment_bytes): written by rcgan_fragments_prepare_dblock2 -- rcgan_fragments_prepare with two more
 * items in the same launch -- from conv2_prepared = Conv2's prepared filter under RCGAN_CONV_OUT_MEANPOOL2 and shortcut_prepared = the
 * 1x1 shortcut's.
 * rcgan_dblock2_bwd (csrc/conv_dblock2_bwd.hip): the block's data gradient as one launch with the same geometry, from dy [n][8][8][128] and
 * the forward's h and x (ReLU masks):
 *   dh = 16bit([h > 0] . (Conv2 + pool)^T(dy));  dxp = 16bit(Shortcut^T(dy));  dx = 16bit(16bit([x > 0] . Conv1^T(dh)) + 0.25 spread2x2(dxp))
 * -- the rounding points of the four launches it replaces (the ConvMeanPool data gradient in its sub-pixel form, rcgan_conv2d_rf backward,
 * the 1x1 data gradient, rcgan_meanpool2_bwd accumulating), and their fp32 summation orders at the training step's shapes, so dh and dx have
 * their bits there.  dh (read by Conv1's filter gradient) and dx are written, dx is not accumulated into; dxp never reaches memory.  It
 * reads two more copies in dblock2_frag (Conv2's summed data-gradient filters, the shortcut's rotated rows), items of the same fragment
 * launch behind the forward's two, whose bytes are unchanged.  Refuses what rcgan_dblock2_ok refuses. */
int rcgan_dblock2_ok(const rcgan_conv_desc* d, const void* conv1_frag, const void* dblock2_frag);
size_t rcgan_dblock2_fragment_bytes(void);
int rcgan_fragments_prepare_dblock2(rcgan_ctx* ctx, const void* const* trunk_prepared, void* trunk_frag, int n, const rcgan_conv_desc* descs,
                                    const void* const* prepared, void* const* frags, const void* conv2_prepared,
                                    const void* shortcut_prepared, void* dblock2_frag);
int rcgan_dblock2_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* conv1_frag, const void* dblock2_frag,
                      const float* bias1, const float* bias2, const float* bias_shortcut, void* h, void* xp, void* y);
int rcgan_dblock2_bwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* h, const void* x, const void* conv1_frag,
                      const void* dblock2_frag, void* dh, void* dx);

/* ---- the 32x32 input block's forward as one launch (csrc/conv_dblock1.hip) ---------------------------------------------------------
 * D.Block.1 of the CIFAR critic (gan_resnet.py:331-353), 32 x 32 x 3 -> 16 x 16 x 128, four workgroups per image (bands of 4 pooled rows):
 *   h = Conv1(x) + b1;  xp = meanpool2(x);  t = Shortcut(xp) + bs;  y = t + meanpool2(Conv2(relu(h)) + b2)
 * with the 16-bit rounding points (h, xp, t, y) and the fp32 summation orders of the three launches it replaces (the image-end
 * small-reduction kernel twice, the gather-form 64 x 64 tile kernel with one K group): every output has their bits.
 * rcgan_dblock1_ok: 1 if d is Conv1's descriptor of exactly that block (3x3, stride 1, no flags, the build's 16-bit dtype, n >= 1) and
 * the fragment copy exists.  dblock1_frag (rcgan_dblock1_fragment_bytes): written by rcgan_fragments_prepare_dblocks --
 * rcgan_fragments_prepare_dblock2 with one more item in the same launch -- from block1_conv2_prepared = D.Block.1.Conv2's prepared filter
 * under RCGAN_CONV_OUT_MEANPOOL2.  conv1_prepared / shortcut_prepared: rcgan_conv_prepare's buffers of Conv1 (d) and of the 1x1 shortcut
 * (n x 16 x 16 x 3 -> 128), whose image-end rows are read in place.  h [n][32][32][128] and y [n][16][16][128] are written, and
 * xp [n][16][16][3] unless it is NULL (the caller holds the pooled images): what the block's (unfused) backward pass reads. */
int rcgan_dblock1_ok(const rcgan_conv_desc* d, const void* dblock1_frag);
size_t rcgan_dblock1_fragment_bytes(void);
int rcgan_fragments_prepare_dblocks(rcgan_ctx* ctx, const void* const* trunk_prepared, void* trunk_frag, int n, const rcgan_conv_desc* descs,
                                    const void* const* prepared, void* const* frags, const void* conv2_prepared,
                                    const void* shortcut_prepared, void* dblock2_frag, const void* block1_conv2_prepared, void* dblock1_frag);
int rcgan_dblock1_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* conv1_prepared, const void* shortcut_prepared,
                      const void* dblock1_frag, const float* bias1, const float* bias2, const float* bias_shortcut, void* h, void* xp, void* y);
/* Fused projection head: pooled features -> psi (D.Output, SN linear d -> 1), label embeddings E = table @ W_e / sigma_e + b_e
 * (embedding.py:29-51 + D.Embedding_y, gan_resnet.py:414-421), logits psi + <feat, E[l]> (:588, :654-660), loss terms and ALL
 * gradients in one launch.  Rows [0, rows_a) form part a, rows [rows_a, n) part b (real | fake of the critic step, :604-606);
 * each part has its loss kind and EITHER int32 labels [rows] (one-hot weights) OR a weight matrix [rows, v] (confusion-matrix
 * rows :682-684, C^-1 rows :647) with optional d/d(weights).  ws: (v*d + n*(v+1) + (v+1)*d + 256) floats of scratch.  loss_acc += weight * (mean over the part's rows);
 * dfeat is written, the five parameter gradients are accumulated (+=); any output may be null.
 * Bounds: n <= 1024, d <= 256, 1 <= v <= 1024.  v <= 16: label embeddings in LDS, parameter gradients may ride (E_pre, defer_ws).
 * v > 16: a route with nothing sized by v in LDS or registers (a thread per output of E, dE and the parameter gradients; the
 * weight-row logits 64 labels at a time): defer_ws is ignored (the gradients are complete on return), E_pre is honoured,
 * ws: (v*d + n*(v+1) + (v+1)*d + n + n*d) floats.  rcgan_proj_head_workspace_bytes(n, d, v) is enough for either route. */
size_t rcgan_proj_head_workspace_bytes(int n, int d, int v);
typedef struct {
  int n, d, v, e_dim;
  int rows_a, kind_a, kind_b;
  float weight;
  const int32_t* labels_a; const float* wts_a; float* dwts_a;
  const int32_t* labels_b; const float* wts_b; float* dwts_b;
  /* Optional (all zero = off): pool the features inside the head -- feat[s][j] = mean over hw of act(x[s][p][j]) (the relu +
   * reduce_mean of gan_resnet.py:405-407) from the trunk's output x [n][hw][d] (x_dtype; d % 128 == 0), and write the gradient
   * straight to dx [n][hw][d] (or NULL).  The `feat` argument is then an OUTPUT buffer [n][d]. */
  const void* x; void* dx;
  int x_dtype, hw, act;
  /* Optional: E [v][d], the label embeddings table @ W_e / sigma_e + b_e computed earlier in the step by
   * rcgan_conv_prepare_batch_embed (they depend on parameters only): the head then starts with its logit kernel. */
  const float* E_pre;
  /* Optional: DEFERRED parameter gradients.  Nothing in the backward pass waits for dw_out / db_out / dtable / dw_e / db_e, so
   * with defer_ws set (>= (n*(v+1) + (v+1)*d) floats that stay untouched until the gradients have been written) the call launches
   * the logit kernel only and leaves the two parameter-gradient launches pending in the context: the next rcgan_dtrunk backward
   * launch carries the first as extra workgroups, the next rcgan_conv2d_bwd_weight_group launch the second, and rcgan_head_flush
   * launches on the spot whatever is still pending (call it before anything reads those gradients).  Same values. */
  void* defer_ws;
  size_t defer_ws_bytes;
} rcgan_head_desc;
int rcgan_proj_head_fwd_bwd(rcgan_ctx* ctx, const rcgan_head_desc* hd, const float* feat, const float* w_out, const float* sigma_out,
                            const float* b_out, const float* table, const float* w_e, const float* sigma_e, const float* b_e,
                            float* loss_acc, float* logits, float* dfeat, float* dw_out, float* db_out, float* dtable, float* dw_e,
                            float* db_e, void* ws, size_t ws_bytes);
int rcgan_head_flush(rcgan_ctx* ctx);

/* ---- LeCam regulariser of the critic's outputs (Tseng et al., "Regularizing Generative Adversarial Networks under Limited Data",
 * CVPR 2021; the two-sided form) ----------------------------------------------------------------------------------------------------
 * Critic cost L_D' = L_D + lambda R,  R = E_real[(D(x, y) - a_F)^2] + E_fake[(D(G(z), y) - a_R)^2], with a_R / a_F exponential moving
 * averages (decay gamma) of the critic's mean output on the real / the fake rows, constants for differentiation.  Each part's
 * expectation is taken exactly as that part's loss term takes it: per logit x the term of loss_kind(x) becomes
 *     t = loss_kind(x) + lambda (x - a)^2,      dt/dx = loss_kind'(x) + 2 lambda (x - a)            (x - a: one fp32 subtraction)
 * and is weighted as before -- the logit at the row's label for a labelled part, mean_rows sum_l w[s,l] (.) for a weight-row part
 * (negative weights included), so every gradient the loss has, the term has (dlogit, dfeat, dx, the parameter gradients, and
 * dwts = gw (loss_kind(x) + lambda (x - a)^2) / rows, gw = weight * gradient scale).
 * rcgan_loss_reg -- all pointers DEVICE, read by the KERNEL: a replayed graph sees the values of the moment it runs:
 *   weight    lambda
 *   anchor_a  the anchor of part a (of the only part of rcgan_loss_reg_fwd_bwd); anchor_b that of part b (head only)
 *   gate      the term is on iff *gate > 0 (NULL: always on); off, it contributes exactly nothing to any output
 *   reg_acc   optional: += the unweighted R of the call (part a + part b, each the mean over its rows); loss_acc += weight * (L + lambda R)
 * reg == NULL, lambda == 0 or a closed gate give the bits of rcgan_loss_fwd_bwd / rcgan_proj_head_fwd_bwd on every output, and those
 * two entry points are the calls below with reg == NULL.  A non-NULL reg needs a finite lambda >= 0, non-NULL 4-byte-aligned anchors
 * (anchor_b only where part b has rows) and 4-byte-aligned gate / reg_acc: anything else is RCGAN_EINVALID_ARG before any launch.
 * The head with reg_acc uses max(256, 2 * cdiv(n, 4)) floats of workspace tail (rcgan_proj_head_workspace_bytes is still enough).
 *
 * rcgan_lecam_update: the controller, one single-workgroup launch after the head.  logits is fp32 [rows_a + rows_b][ld]; part a is
 * rows [0, rows_a), part b the rest.  The score of a row is the logit itself (ld == 1, neither labels nor weights), the logit at its
 * label (a label outside [0, ld) makes the row count as zero and read nothing; it stays in the denominator), or sum_l w[s,l] logit[s,l]
 * (weight rows [rows][ld]).  m_a, m_b = the batch means of the scores: fp32 sums in a fixed order, no atomics.
 * state: DEVICE float[8] = {a_R, a_F, updates, mean_real_last, mean_fake_last, skipped, 0, 0}; part a holds the real rows.  A call:
 *   m_a or m_b not finite:  skipped += 1, nothing else changes;
 *   updates == 0:           a_R = m_a, a_F = m_b;
 *   otherwise:              a_R = decay * a_R + (1 - decay) * m_a (two products, one sum, in fp32), a_F likewise from m_b;
 *   then mean_real_last = m_a, mean_fake_last = m_b, updates += 1.
 * The real part's loss is pulled towards a_F (anchor = state + 1), the fake part's towards a_R (state + 0); gate = state + 2.
 * rows_a, rows_b >= 1, ld >= 1, logits / state non-NULL, every pointer 4-byte aligned, per part at most one of labels / weights and
 * exactly one when ld > 1, decay in [0, 1]: anything else is RCGAN_EINVALID_ARG and launches nothing. */
typedef struct {
  float weight;
  const float* anchor_a; const float* anchor_b;
  const float* gate;
  float* reg_acc;
} rcgan_loss_reg;
int rcgan_loss_reg_fwd_bwd(rcgan_ctx* ctx, int kind, int rows, int cols, const float* x, const float* wts, float weight,
                           float* loss_acc, float* dlogit, float* dwts, const rcgan_loss_reg* reg);
int rcgan_proj_head_reg_fwd_bwd(rcgan_ctx* ctx, const rcgan_head_desc* hd, const float* feat, const float* w_out, const float* sigma_out,
                                const float* b_out, const float* table, const float* w_e, const float* sigma_e, const float* b_e,
                                float* loss_acc, float* logits, float* dfeat, float* dw_out, float* db_out, float* dtable, float* dw_e,
                                float* db_e, void* ws, size_t ws_bytes, const rcgan_loss_reg* reg);
int rcgan_lecam_update(rcgan_ctx* ctx, int rows_a, int rows_b, const float* logits, int ld, const int32_t* labels_a, const float* wts_a,
                       const int32_t* labels_b, const float* wts_b, float* state, float decay);
/* (bce_onehot: one workgroup, any rows x cols, labels in [0, cols); loss_acc and dx may be NULL.) */
int rcgan_bce_onehot_fwd_bwd(rcgan_ctx* ctx, int rows, int cols, const float* x, const int32_t* labels,
                             float weight, float* loss_acc, float* dx);
/* recover_labels objective (mnist/model.py:533-537): gen [r*ydim, pix] = one generated image per (real sample r, label y),
 * actual [r, pix], yrec [r, ydim] = softmax of the recovered label logits.
 *   loss = mean_r sum_y yrec[r,y] * mean_pix (actual[r] - gen[r,y])^2
 * Writes loss [1], dgen (same shape as gen, or NULL) and dyrec [r, ydim] (or NULL).  ws: r*ydim floats = rcgan_recover_mse_workspace_bytes(r, ydim). */
size_t rcgan_recover_mse_workspace_bytes(int r, int ydim);
int rcgan_recover_mse_fwd_bwd(rcgan_ctx* ctx, int r, int ydim, int pix, int dtype, const void* gen, const void* actual,
                              const float* yrec, float* loss, void* dgen, float* dyrec, void* ws, size_t ws_bytes);
/* C = softmax(logits) row-wise and its adjoint (gan_resnet.py:522, mnist/model.py:106).  A thread per row: any cols (the
 * K x K confusion matrix of rcgan-u, K <= 1024). */
int rcgan_softmax_rows_fwd(rcgan_ctx* ctx, int rows, int cols, const float* logits, float* p);
int rcgan_softmax_rows_bwd(rcgan_ctx* ctx, int rows, int cols, const float* p, const float* dp, float* dlogits,
                           int accumulate);

/* ---- diversity-sensitive generator term on same-label pairs (csrc/diversity.hip; Yang et al., "Diversity-Sensitive Conditional
 * GANs", ICLR 2019; Mao et al., "Mode Seeking GANs", CVPR 2019; the linear clamped form, as StarGAN v2 uses it) ---------------------
 * x [2P, D] and z [2P, Z] in `dtype` (RCGAN_F32 or the library's 16-bit type); pair i is rows (i, i + P).  One launch, one workgroup
 * per pair:
 *   dI_i = (1/D) sum_k |x[i,k] - x[i+P,k]|,   dz_i = (1/Z) sum_k |z[i,k] - z[i+P,k]|,   r_i = dI_i / dz_i      (fp32)
 *   m_i  = 0 if labels != NULL and labels[i] != labels[i+P], or if dz_i == 0; else 1
 *   *loss_acc   += -(weight / P) sum_i m_i min(r_i, tau)      the divisor is always P: masked pairs stay in the denominator
 *   ratio_out[i] = r_i, or exactly -1 for a masked pair
 *   c_i = m_i [r_i < tau] weight g / (P D dz_i),  g = the scale of rcgan_set_grad_scale (host value times the device value, read by
 *         the kernel); the loss VALUE is never scaled
 *   dx[i,k] (= | +=) -c_i sgn(x[i,k] - x[i+P,k]),  dx[i+P,k] (= | +=) +c_i sgn(x[i,k] - x[i+P,k]),  sgn(0) = 0
 * A pair at or above the clamp and a masked pair write zeros with accumulate = 0 and leave dx bit for bit untouched with
 * accumulate = 1.  z gets no gradient.  tau = +inf: no clamp.  loss_acc, dx, ratio_out and labels may each be NULL.
 * Both rows of a pair are read once and their differences stay in registers (16-byte loads and stores: a row is a whole number of
 * 16-byte chunks, at most 1024 of them, and x and dx are 16-byte aligned) or, on the element-wise route every other case takes,
 * their signs stay in LDS (D <= 61440 there; longer rows: RCGAN_EUNSUPPORTED_SHAPE).  The sums are fixed-order block reductions; the P
 * loss terms are per-pair floats in ws, summed in pair order by the last workgroup to arrive: no floating-point atomics, the same
 * bits on every run, eager or replayed.  ws: rcgan_pair_diversity_workspace_bytes(P), needed only with a loss_acc
 * (RCGAN_EWORKSPACE_TOO_SMALL otherwise).
 * P, D, Z >= 1; x, z non-NULL and element-aligned, dx element-aligned; labels, loss_acc, ratio_out, ws 4-byte aligned; weight finite
 * and >= 0; tau > 0 (not NaN); a known dtype: anything else is RCGAN_EINVALID_ARG before any launch.  weight == 0 launches nothing and
 * touches nothing. */
size_t rcgan_pair_diversity_workspace_bytes(int pairs);
int rcgan_pair_diversity_fwd_bwd(rcgan_ctx* ctx, int pairs, int d, int zdim, int dtype, const void* x, const void* z, const int32_t* labels,
                                 float weight, float tau, float* loss_acc, void* dx, int accumulate, float* ratio_out, void* ws,
                                 size_t ws_bytes);

/* ---- balanced consistency regularisation of the critic (csrc/loss.hip; Zhang et al., "Consistency Regularization for Generative
 * Adversarial Networks", ICLR 2020; Zhao et al., "Improved Consistency Regularization for GANs", 2020: the balanced form, bCR) -------
 * With the option on a critic step evaluates the trunk on 4B rows: rows [0, 2B) are the [real ; fake] the critic sees anyway (through
 * DiffAugment or its gated form where those are on), rows [2B, 4B) are rcgan_diffaugment_fwd(x_all, u_bcr, bcr_policy) of the
 * UN-augmented [real ; fake]: always applied (no gate), one independent row of u_bcr per image.  The critic cost gains
 *     L_bcr = lam_real * mean_{i < B} c_i  +  lam_fake * mean_{B <= i < 2B} c_i,
 * c_i the squared difference of row i's score and row (i + 2B)'s, both scores formed at row i's own label or weight row, exactly as
 * that part's loss term forms its expectation (the rule of the LeCam section above):
 *     labelled part   c_i = (logit[i, y_i] - logit[i + 2B, y_i])^2
 *     weighted part   c_i = sum_l w[i, l] (logit[i, l] - logit[i + 2B, l])^2        (negative weights included)
 * Both members of a pair get a gradient, and so do weight rows that require one.  The term has no state.
 *
 * rcgan_pair_consistency_fwd_bwd: ONE part per call, one single-workgroup launch.  x and x_aug are fp32 [pairs][cols]: cols == 1 for
 * a labelled part whose logit is already taken at the label, the class count for a weighted one.  wts: fp32 [pairs][cols], or NULL
 * (every weight 1).  With e = x[i,l] - x_aug[i,l] (one fp32 subtraction), w = wts[i,l] or 1:
 *     m = (1 / pairs) sum_i sum_l w e^2            (fp32, a thread's elements in order, then a fixed-order block sum: no atomics)
 *     *loss_acc += lam * m;    *term_acc += m      (the unweighted mean, for reports; may be NULL, as loss_acc may)
 *     dx[i,l]    (= | +=)  g lam 2 w e / pairs     (accumulate = 0 | 1: the hinge terms have already WRITTEN x's gradient)
 *     dx_aug[i,l] =       -g lam 2 w e / pairs     (always written whole)
 *     dwts[i,l] +=         g lam e^2 / pairs       (always accumulated)
 * g = the scale of rcgan_set_grad_scale (host value times the device value, read by the kernel); the loss VALUE is never scaled.
 * dx, dx_aug and dwts may each be NULL (dwts needs wts).  Identical rows give exactly 0 everywhere.  The same bits on every run, eager
 * or replayed.  pairs >= 1, cols >= 1, pairs * cols <= 2^20 (one workgroup serves them all); x and x_aug non-NULL; every pointer 4-byte aligned; lam finite and >= 0:
 * anything else is RCGAN_EINVALID_ARG before any launch.  lam == 0 launches nothing and touches nothing. */
int rcgan_pair_consistency_fwd_bwd(rcgan_ctx* ctx, int pairs, int cols, const float* x, const float* x_aug, const float* wts, float lam,
                                   float* loss_acc, float* term_acc, float* dx, int accumulate, float* dx_aug, float* dwts);

/* ---- training the generated-label-accuracy classifier (csrc/classifier.hip; fp32 model, classifier.py) -------------------- */
/* Sparse softmax cross-entropy (tf.nn.sparse_softmax_cross_entropy_with_logits + reduce_mean), one launch:
 *   *loss_acc      += weight * mean_rows(-log softmax(logits)[label])
 *   *n_correct_acc += the number of rows whose arg-max (lowest index on ties) equals the label   (fp32 scalar; may be NULL)
 *   dlogits         = weight * (softmax - onehot) / rows, times the scale of rcgan_set_grad_scale   (may be NULL: evaluation)
 * cols 2..1024, any rows; max-subtracted, log-sum-exp in fp32.  A wavefront per row; the sums over rows are per-workgroup partials
 * in ws finished in workgroup order by the last workgroup to arrive (no floating-point atomics: the same bits run to run).
 * ws: rcgan_softmax_xent_workspace_bytes(rows).  A label outside [0, cols) contributes nothing. */
size_t rcgan_softmax_xent_workspace_bytes(int rows);
int rcgan_softmax_xent_fwd_bwd(rcgan_ctx* ctx, int rows, int cols, const float* logits, const int32_t* labels, float weight,
                               float* loss_acc, float* n_correct_acc, float* dlogits, void* ws, size_t ws_bytes);
/* Forward-corrected cross-entropy for NOISY labels (Patrini et al. 2017), the same launch shape, workspace and determinism:
 *   *loss_acc      += weight * mean_rows(-log((softmax(logits) . C)[label]))
 *   *n_correct_acc += the number of rows whose arg-max (lowest index on ties) equals the (noisy) label          (may be NULL)
 *   posterior[r][y] = softmax(logits[r])[y] * C[y][label_r] / (softmax(logits[r]) . C)[label_r]    [rows, cols] (may be NULL)
 *   recovered[r]    = arg-max_y posterior[r][y], lowest index on ties                              [rows] int32 (may be NULL)
 *   dlogits         = weight * (softmax - posterior) / rows, times the scale of rcgan_set_grad_scale            (may be NULL)
 * ct: [cols, cols] fp32, the TRANSPOSE of the confusion matrix: ct[noisy][clean] = C[clean][noisy] = P(noisy | clean).  Max-subtracted
 * twice (over the row, and over the support of ct[label]), so nothing underflows to log 0; with C = I every output that
 * rcgan_softmax_xent_fwd_bwd has is that entry's, bit for bit, for in-range labels.  A row whose label is outside [0, cols) or whose
 * ct row has no positive entry contributes nothing to the loss (still divided by ALL rows) and gets a zero gradient row, a zero
 * posterior row and recovered = -1. */
int rcgan_softmax_xent_forward_fwd_bwd(rcgan_ctx* ctx, int rows, int cols, const float* logits, const int32_t* labels, const float* ct,
                                       float weight, float* loss_acc, float* n_correct_acc, float* dlogits, float* posterior,
                                       int32_t* recovered, void* ws, size_t ws_bytes);
/* The option-A shortcut of the classifier's down-sampling blocks as one launch each way: y[n, h/2, w/2, 2c] = the 2x2 mean of
 * x[n, h, w, c] in channels [c/2, c/2 + c), zeros elsewhere -- the bits of rcgan_meanpool2_fwd followed by rcgan_pad_channels
 * without the intermediate tensor.  Backward: dx (=|+=) the middle channels of dy, a quarter to each of the four pixels.
 * h, w, c even. */
int rcgan_shortcut_a_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y);
int rcgan_shortcut_a_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* dy, void* dx, int accumulate);
/* tf.train.MomentumOptimizer on a flat fp32 range with L2 weight decay on its first decay_count elements:
 *   g' = grad_scale * g + weight_decay * w   (i < decay_count;  grad_scale * g for the rest)
 *   accum = momentum * accum + g';   w -= lr * accum,   or with nesterov   w -= lr * (g' + momentum * accum)
 * hyper: DEVICE float[1] = {lr}, read at execution time (a captured step follows the schedule, as with rcgan_adam_tf). */
int rcgan_sgd_momentum(rcgan_ctx* ctx, size_t count, size_t decay_count, float* w, const float* g, float* accum, const float* hyper,
                       float momentum, float weight_decay, int nesterov, float grad_scale);
/* The classifier's input pipeline over a data set resident on the device: images_chw_u8 [n_images][3][32][32] bytes, labels_all
 * [n_images].  Sample i = image index[i] translated by (shift_flip[i][0], shift_flip[i][1]) pixels down / right (each clamped to
 * [-pad, pad], zeros shifted in), then mirrored left-right when shift_flip[i][2] != 0, written as raw pixel values 0..255 in NHWC in
 * `dtype`; labels_out[i] = labels_all[index[i]] (either may be NULL).  An index outside [0, n_images) gives a zero image, label -1. */
int rcgan_augment_cifar(rcgan_ctx* ctx, int n, int n_images, const uint8_t* images_chw_u8, const int32_t* labels_all,
                        const int32_t* index, const int32_t* shift_flip, int pad, int dtype, void* y_nhwc, int32_t* labels_out);
/* The MNIST label classifier (mnist_classifier.py) stands in for the reference's frozen mnist/mnist_dcnn/graph_optimized.pb
 * (mnist/utils.py:276-298: input `x`, a dropout keep-probability placeholder, output `pred_class`): the "deep MNIST" convnet.  Its two
 * memory-bound operators follow.  Each returns RCGAN_EINVALID_ARG, before it launches anything, for a non-positive dimension or count,
 * odd h or w, a NULL tensor, a keep_prob outside (0, 1] or not finite, or an unknown dtype (RCGAN_F32 and the library's 16-bit type are
 * taken).  Inputs are assumed finite; x and y must not alias. */
/* y[n,h/2,w/2,c] = maxpool2x2_stride2(relu(x[n,h,w,c]))  -- the graph's tf.nn.relu + tf.nn.max_pool(ksize 2, strides 2, SAME) pair
 * after each convolution, one launch; h, w even.  Pure selection: y holds the bits of an element of x, or +0. */
int rcgan_relu_maxpool2_fwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, void* y);
/* dx (= | +=): dy goes to the FIRST maximum of each window in the order (0,0),(0,1),(1,0),(1,1) if that maximum is > 0,
 * nothing otherwise; every element of dx is written (zeros included) when accumulate == 0.  Recomputed from x: no saved index.
 * The gradient tf.gradients forms through MaxPoolGrad + ReluGrad, except at ties, where this rule is the documented one.
 * accumulate != 0: dx = old + contribution in fp32, rounded once to the stored type. */
int rcgan_relu_maxpool2_bwd(rcgan_ctx* ctx, int n, int h, int w, int c, int dtype, const void* x, const void* dy, void* dx,
                            int accumulate);
/* tf.nn.dropout(x, keep_prob) in front of the graph's last dense layer.
 * Element i is kept iff u_i < keep_prob, u_i the i-th number of the stream rcgan_rng_fill(kind 0, lo 0, hi 1) draws from
 * (seed, state): u = (r >> 8) * 2^-24 of word i.  y = x * scale if kept, else 0, with scale = 1.0f / keep_prob formed in fp32 on the
 * host (the product in fp32, rounded once to the stored type); mask[i] = 1 / 0 (count bytes, caller-owned).  state: DEVICE
 * uint64[1] stream offset, or NULL for offset 0.  The stream advances by ceil(count / 4) quads, on the stream, as rcgan_rng_fill
 * does (a replayed graph draws a fresh mask).  keep_prob in (0, 1]; at 1.0 everything is kept and the stream still advances. */
int rcgan_dropout_fwd(rcgan_ctx* ctx, size_t count, int dtype, float keep_prob, uint64_t seed, void* state, const void* x, void* y,
                      uint8_t* mask);
/* dx (= | +=) dy * scale where mask[i] != 0, 0 elsewhere: the product rounded to fp32, then (accumulate != 0) added to the old value in
 * fp32, the result rounded once to the stored type. */
int rcgan_dropout_bwd(rcgan_ctx* ctx, size_t count, int dtype, float keep_prob, const uint8_t* mask, const void* dy, void* dx,
                      int accumulate);

/* ---- differentiable augmentation of the critic's input (csrc/augment.hip; Zhao et al., "Differentiable Augmentation for
 * Data-Efficient GAN Training", NeurIPS 2020) --------------------------------------------------------------------------------
 * y = A_u(x) over NHWC images x[n, h, w, 3] (fp32 or the library's 16-bit dtype), and the adjoint of that map.  Nothing random
 * happens inside: u[n][8] holds eight fp32 uniforms in [0, 1) per sample, drawn by the caller (rcgan_rng_fill, kind 0), and both
 * entry points are pure functions of (images, u, policy).  policy is a mask of the RCGAN_AUG_* bits; a step whose bit is clear is
 * skipped (policy 0: a copy).  Per sample, in this order, all arithmetic in fp32, the output rounded once to `dtype`:
 *   COLOR        b = u0 - 0.5, s = 2 u1, k = u2 + 0.5
 *                brightness  x1 = x + b
 *                saturation  x2 = (x1 - m) s + m,   m[p][q] = mean of x1[p][q][:] over the 3 channels
 *                contrast    x3 = (x2 - M) k + M,   M = mean of x2 over all h w 3 values of the sample
 *   TRANSLATION  S_h = (h + 4) / 8, S_w = (w + 4) / 8 (integer division: 4 pixels of 32);
 *                ty = min(floor(u3 (2 S_h + 1)), 2 S_h) - S_h, tx likewise from u4 and S_w (the product in fp32)
 *                x4[p][q] = x3[p + ty][q + tx] where that pixel exists, 0 elsewhere
 *   CUTOUT       oy = min(floor(u5 (h + 1)), h), ox likewise from u6 and w
 *                rows max(oy - h/4, 0) .. min(oy + h/4 - 1, h - 1) x columns max(ox - w/4, 0) .. min(ox + w/4 - 1, w - 1) are set to 0
 *                (a window of h/2 x w/2 pixels, clipped at the border)
 *   u7 is reserved and ignored (the gates of the adaptive probability live in a buffer of their own, gate_u: see below).
 * y_pool (may be NULL): [n, h/2, w/2, 3], the 2x2 mean of the STORED y -- the bits rcgan_meanpool2_fwd gives on y -- out of the
 * same launch (D.Block.1's shortcut reads the pooled critic input, gan_resnet.py:346).
 * Backward: dx (=|+=) A_u^T dy.  The map is affine in x, so the adjoint needs u only: dy is masked by the cutout window, shifted by
 * (-ty, -tx) with zero fill (g3), then g2 = k g3 + (1 - k) mean_all(g3) and dx = s g2 + (1 - s) mean_c(g2); the brightness offset has
 * no term.  Without COLOR the pixels that are cut out or shifted out of the frame get exactly 0.
 * One workgroup per sample, the sample in LDS; the means are summed in a fixed order (no floating-point atomics): the same bits on
 * every run, eager or replayed.  h and w multiples of 4, 2 h w 3 floats (the sample and its transform) within the 160 KiB of LDS of a compute unit (up to 80 x 80), n >= 1, image pointers
 * aligned to four elements; anything else is RCGAN_EINVALID_ARG. */
#define RCGAN_AUG_COLOR 1
#define RCGAN_AUG_TRANSLATION 2
#define RCGAN_AUG_CUTOUT 4
int rcgan_diffaugment_fwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* x, const float* u, void* y,
                          void* y_pool);
int rcgan_diffaugment_bwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* dy, const float* u, void* dx,
                          int accumulate);

/* ---- adaptive augmentation probability on top of the above (csrc/augment.hip; Karras et al., "Training Generative Adversarial
 * Networks with Limited Data", NeurIPS 2020) -------------------------------------------------------------------------------------
 * Every transform of `policy` is applied to a sample with probability p, and p follows r = E[sign D(real)] towards a target.
 * u7 stays reserved: the gates live in a buffer of their own, gate_u[n][4], fp32 uniforms in [0, 1) drawn by the caller; column 0
 * gates COLOR, 1 TRANSLATION, 2 CUTOUT, column 3 is reserved and ignored.
 *   rcgan_diffaugment_gated_fwd   sample i is transformed exactly as rcgan_diffaugment_fwd transforms it under
 *       policy_i = policy & sum_t (gate_u[i][t] < *p_dev ? bit_t : 0)        (strict <, in fp32: p = 1 applies everything,
 *       p = 0 nothing, a NaN p nothing), y and y_pool (may be NULL) get the same bits, and policy_i is written to sample_policy[i]
 *       (DEVICE int32[n]).  p_dev is a DEVICE float*, read by the KERNEL: a captured launch sees the value of the moment it runs.
 *   rcgan_diffaugment_sampled_bwd the adjoint under the policies the forward recorded: sample i gets the bits of
 *       rcgan_diffaugment_bwd under sample_policy[i] (only its three RCGAN_AUG_* bits are looked at).  It takes neither gate_u nor
 *       p, so a change of p between a forward and its backward cannot make the two disagree.
 *   rcgan_ada_update              the controller, one single-workgroup launch.  logits is fp32 [n][ld]; the score of row i is
 *       s_i = logits[i * ld + (labels ? labels[i] : 0)]; a row whose label is outside [0, ld) counts as ZERO (nothing is read for
 *       it), though it still counts as an image.  sign(s) = (s > 0) - (s < 0): +-0 and NaN count 0, +-inf count +-1.
 *       ada_state: DEVICE float[8] = {p, sign_sum, image_count, steps, r_last, updates, 0, 0}.  A call performs
 *       sign_sum += sum_i sign(s_i), image_count += n, steps += 1, and when steps == interval then, in this order, all in fp32:
 *       r_last = sign_sum / image_count;  p = clamp(p + sign(r_last - target) * image_count / images, 0, 1);  updates += 1;
 *       sign_sum = image_count = steps = 0.  (The sum of signs is a sum of small integers: any reduction order is exact.)
 * Besides the conditions of rcgan_diffaugment_fwd: gate_u, p_dev, sample_policy non-NULL and 4-byte aligned; for the update
 * n >= 1, ld >= 1, interval >= 1, images > 0, logits / ada_state non-NULL and 4-byte aligned (labels 4-byte aligned).  Anything
 * else is RCGAN_EINVALID_ARG and launches nothing. */
int rcgan_diffaugment_gated_fwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, int policy, const void* x, const float* u,
                                const float* gate_u, const float* p_dev, void* y, void* y_pool, int32_t* sample_policy);
int rcgan_diffaugment_sampled_bwd(rcgan_ctx* ctx, int n, int h, int w, int dtype, const void* dy, const float* u,
                                  const int32_t* sample_policy, void* dx, int accumulate);
int rcgan_ada_update(rcgan_ctx* ctx, int n, const float* logits, int ld, const int32_t* labels, float* ada_state, float target,
                     float images, int interval);

/* ---- per-class moments of a feature stream (csrc/moments.hip; the Frechet distance of frechet.py) ------------------------------
 * state (caller-owned, zeroed once by the caller, rcgan_class_moments_bytes(d, n_classes) bytes, 8-byte aligned), all fp64:
 *   count[K], sum[K][d], sumsq[K][d][d] = the full matrix sum of x x^T over the rows of each class, then ONE counter of rejected rows.
 * Every call adds a batch feat[n][d] (fp32) with labels[n]; labels may be NULL only with n_classes == 1 (every row is class 0).  A
 * label outside [0, K) writes nowhere: its row is skipped and the rejected counter goes up by one.
 * One launch on the context's stream, no host synchronisation, legal inside a captured graph.  The product of two fp32 values is
 * exact in fp64; every entry is summed by one owner thread in row order and then added to the state (no floating-point atomics): the
 * same bits on every run, and an error of at most n 2^-52 sum|x_i x_j| per entry.
 * 1 <= d <= 256, 1 <= n_classes <= 1024, n >= 1, non-NULL feat / state: anything else is RCGAN_EINVALID_ARG before any launch (a
 * NULL context included, so the checks need no device); rcgan_class_moments_bytes returns 0 for a d or n_classes outside the bounds. */
size_t rcgan_class_moments_bytes(int d, int n_classes);
int rcgan_class_moments_accum(rcgan_ctx* ctx, int n, int d, int n_classes, const float* feat, const int32_t* labels, void* state);

/* ---- k-nearest-neighbour radii and ball queries on feature rows (csrc/knn.hip; precision / recall / density / coverage of manifold.py)
 * Rows [n][d] (fp32) are grouped into n_seg contiguous segments by an int32 DEVICE array off[n_seg + 1] (off[0] = 0, off[n_seg] = n,
 * non-decreasing): one segment for a pooled metric, one per class for a per-class one.  Segment s of the queries only ever meets
 * segment s of the references.  The kernel does not trust the array: every offset is clamped to [0, n] and off[s + 1] < off[s] is an
 * empty segment, so a bad array gives wrong numbers (and rows outside every segment are not written) but never an access outside the
 * tensors.  With a well-formed array every output row is written on every call.
 * A squared distance is the fp32 sum of (a_i - b_i)^2 over ascending i, every term non-negative -- not |a|^2 + |b|^2 - 2 a.b, which
 * loses a threshold comparison to cancellation: |computed - exact| <= (d + 3) 2^-24 exact.  (Hence vector fp32, not the matrix cores.)
 * One launch each on the context's stream, no workspace, no host synchronisation, legal inside a captured graph; an order statistic,
 * an integer count and a minimum do not depend on the merge order (no floating-point atomics): the same bits on every run.
 * 1 <= d <= 256, 1 <= k <= 16, n, nq, nr >= 1, 1 <= n_seg <= 1024, required pointers non-NULL: anything else is RCGAN_EINVALID_ARG
 * before any launch (a NULL context included, so the checks need no device).
 *
 * radius2[i] = the (k+1)-th smallest of { ||x_i - x_j||^2 : j in the segment of i, j = i included }
 *            = squared distance to the k-th nearest OTHER row, duplicates counted;
 *              -1.0f for every row of a segment with <= k rows. */
int rcgan_knn_radius(rcgan_ctx* ctx, int n, int d, int k, int n_seg, const float* x, const int32_t* off, float* radius2);
/* For query row i of segment s, over the reference rows j of segment s:
 *   count[i]    = #{ j : ||q_i - r_j||^2 <= r_radius2[j] }   (a negative radius never matches)
 *   nearest2[i] = min_j ||q_i - r_j||^2                      (+inf for an empty reference segment)
 * count and nearest2 may each be NULL; r_radius2 may be NULL only when count is. */
int rcgan_ball_query(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const float* q, const int32_t* q_off, const float* r,
                     const int32_t* r_off, const float* r_radius2, int32_t* count, float* nearest2);

/* ---- row sums of the cubic polynomial kernel (csrc/ksum.hip; the unbiased MMD^2 "kernel distance" of kid.py)
 * rowsum[i] = sum over the reference rows j of query row i's segment of (gamma * <q_i, r_j> + coef0)^3, fp64;
 * exclude_same_row != 0 leaves out j == i (global row indices: meaningful when q and r are the same rows and offsets).
 * Segments as above: int32 DEVICE arrays q_off / r_off [n_seg + 1], every offset clamped to [0, n], a decreasing pair an empty
 * segment, segment s of the queries meets only segment s of the references, rows outside every segment are not written, an empty
 * reference segment gives 0.0.
 * Arithmetic: the inner product is fp32 on the matrix cores (v_mfma_f32_32x32x2_f32, a chain of fused multiply-adds in an order of
 * the kernel's choosing): |dot_c - dot| <= g_d * sum_i |q_i r_i|, g_d = d u / (1 - d u), u = 2^-24.  Everything after it is fp64:
 * t = gamma * (double)dot_c + coef0 (one fused multiply-add), then t * t * t, then the row sum.  No floating-point atomics: the order
 * in which a row's terms are added is fixed by the launch geometry, so the same bits come out on every run, eager or replayed.
 * One launch on the context's stream, no workspace, no host synchronisation, legal inside a captured graph.
 * 1 <= d <= 256, nq, nr >= 1, 1 <= n_seg <= 1024, finite gamma and coef0, non-NULL pointers (rowsum 8-byte aligned): anything else
 * is RCGAN_EINVALID_ARG before any launch (a NULL context included, so the checks need no device). */
int rcgan_poly3_rowsum(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const float* q, const int32_t* q_off, const float* r,
                       const int32_t* r_off, double gamma, double coef0, int exclude_same_row, double* rowsum);

/* ---- per-scale SSIM means of image pairs (csrc/msssim.hip; the intra-class MS-SSIM of msssim.py)
 * x: n images [n][h][w][c], NHWC, raw pixels 0..255 (uint8, DEVICE); pairs: int32 DEVICE array [n_pairs][2] of image indices.
 * For pair p = (i, j) and scale l = 0..4 (the image, then four times the 2 x 2 mean at stride 2 anchored at (0, 0), the last row /
 * column averaged with itself where a size is odd: sizes ceil(h_l / 2)):
 *   out[p][0][l] = the mean over positions and channels of the contrast-structure map v1 / v2,
 *   out[p][1][l] = the mean of the full SSIM map (2 mu_i mu_j + c1) v1 / ((mu_i^2 + mu_j^2 + c1) v2),
 * v1 = 2 sigma_ij + c2, v2 = sigma_ii + sigma_jj + c2, c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2, the local moments taken under a
 * Gaussian window of s = min(11, h_l, w_l) taps per side with sigma = 1.5 s / 11 (centres k - (s - 1) / 2, normalised), 'valid'
 * positions only: _SSIMForMultiScale of the reference's cifar10/common/msssim.py for a batch of one, level by level as its
 * MultiScaleSSIM walks them.  The combination over scales and pairs is the host's (msssim.combine).
 * A pair with an index outside [0, n) gets nan in its ten outputs and touches nothing else; there is never an access outside the
 * tensors.
 * Arithmetic: fp32, the taps computed in float64 on the host; variances and the covariance are sums of non-negative (for the
 * covariance: Cauchy-Schwarz bounded) centred terms, never a difference of two second moments, and every sum is taken in an order
 * fixed by the launch geometry (no floating-point atomics): the same bits on every run, eager or replayed.
 * |out - exact| <= 1e-4 for every pair and scale (derivation: the header of csrc/msssim.hip); identical images give exactly 1.
 * One launch on the context's stream (one workgroup per pair), no workspace, no host synchronisation, legal inside a captured graph.
 * c 1 or 3, 16 <= h, w <= 32 (five levels exist from 16 on; both images, their pyramids and one channel's filtered fields stay in
 * LDS up to 32), n, n_pairs >= 1, non-NULL pointers (pairs and out 4-byte aligned): anything else is RCGAN_EINVALID_ARG before any
 * launch (a NULL context included, so the checks need no device). */
int rcgan_msssim_pairs(rcgan_ctx* ctx, int n, int h, int w, int c, int n_pairs, const uint8_t* x, const int32_t* pairs, float* out);

/* ---- nearest reference image of every query image, in pixel space (csrc/nn_u8.hip; the memorisation metrics of neighbours.py)
 * q[nq][d], r[nr][d]: raw pixels 0..255 (uint8, DEVICE), rows in any fixed pixel order that is the same on both sides.
 *   best[i] = min over the reference rows j of query row i's segment of ((uint64)dist2(i, j) << 32 | (uint32)j),
 *   dist2(i, j) = sum_k (q[i][k] - r[j][k])^2, EXACT (what int64 arithmetic gives), j the global reference row.
 * The packing is the tie rule: among equally near rows the lowest index wins.  exclude_same_row != 0 leaves out j == i (global row
 * indices: meaningful when q and r are the same rows and offsets).  0xFFFFFFFFFFFFFFFF where no candidate exists: an empty reference
 * segment, a one-row segment with exclusion.
 * Segments as above: int32 DEVICE arrays q_off / r_off [n_seg + 1], every offset clamped to [0, n], a decreasing pair an empty
 * segment, segment s of the queries meets only segment s of the references, rows outside every segment are not written, and there is
 * never an access outside the tensors.
 * Arithmetic: both operands centred (x ^ 0x80 read as int8 is x - 128), dist2 = |a|^2 + |b|^2 - 2 a.b in int32 with the inner
 * products on the integer matrix cores (v_mfma_i32_32x32x32_i8); no intermediate reaches 2^31 for d <= 12288 (derivation: the header
 * of csrc/nn_u8.hip).  A minimum of integers does not depend on the merge order (the reference range of a query is split over
 * workgroups that merge with one 64-bit integer atomic minimum per row; no floating-point atomics): the same bits on every run, eager
 * or replayed, and for every way the work is split.
 * Two launches (fill of the rows inside a segment, kernel) on the context's stream, no workspace, no host synchronisation, legal
 * inside a captured graph.
 * 16 <= d <= 12288 and d a multiple of 16, q and r 16-byte aligned (rows are 16-byte loads), nq, nr >= 1, 1 <= n_seg <= 1024,
 * non-NULL pointers (offsets 4-byte, best 8-byte aligned): anything else is RCGAN_EINVALID_ARG before any launch (a NULL context
 * included, so the checks need no device). */
int rcgan_nn_u8(rcgan_ctx* ctx, int nq, int nr, int d, int n_seg, const uint8_t* q, const int32_t* q_off, const uint8_t* r,
                const int32_t* r_off, int exclude_same_row, uint64_t* best);

/* ---- sliced Wasserstein distance on Laplacian-pyramid patch descriptors (csrc/swd.hip; the pixel-space distance of swd.py)
 * x: n images [n][h][w][c], NHWC, raw pixels 0..255 (uint8, DEVICE), sorted by segment; off: int32 DEVICE array [n_seg + 1], every
 * offset clamped to [0, n], a decreasing pair an empty segment, an image outside every segment (or in several: the lowest one counts)
 * is read but never written for; a bad array gives wrong numbers and never an access outside the tensors.
 * The pyramid: G0 = x, G1 = down(G0), G2 = down(G1); L0 = G0 - up(G1), L1 = G1 - up(G2), L2 = G2.  down: the taps [1,4,6,4,1]/16
 * along each axis under the mirror boundary that does not repeat the edge (-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3), even
 * indices kept; up: zero-insert to twice the size, then [1,4,6,4,1]/8 along each axis, the same boundary.  Level `level` of an
 * image has (h >> level) x (w >> level) pixels; its descriptors are the 7 x 7 x c neighbourhoods centred on y = 3, 3 + stride, ...
 * <= (h >> level) - 4, likewise x (n_pos per image, at most 49), elements in the order (dy, dx, channel).
 *
 * rcgan_swd_moments: mom[s][ch] = {sum, sum of squares} (fp64) of channel ch over ALL descriptor entries of segment s -- a pixel
 *   counts once per descriptor that covers it; zeros for an empty segment.  part: fp64 DEVICE scratch of the caller, [n][c][2],
 *   overwritten (the per-image sums: the call is two launches, images then segments).  Every sum is fp64 in an order fixed by the
 *   launch geometry, no floating-point atomics.
 * rcgan_swd_project: proj[d][s][j * n_pos + p] (fp32, [n_dir][n_seg][width]) = the dot product of direction dirs[d] (fp32,
 *   [n_dir][49 c]) with descriptor p of the j-th image of segment s, normalised per channel with the segment's mean and 1 / deviation
 *   (ddof 0), both derived on the device from `mom` as S / N and 1 / sqrt(Q / N - (S / N)^2) in fp64 and rounded to fp32; 1 / deviation
 *   := 0 where that variance is not positive.  Every entry at or behind the segment's descriptor count is +inf; entries that would
 *   fall behind `width` are dropped.  1 + ceil(n_dir / 128) launches.
 *   Arithmetic: the pyramid in fp32 (L0, L2, G1, G2 exact; |L1 - exact| <= delta_1 = 7 u 255, u = 2^-24), centring and scaling in
 *   fp32, the dot product a chain of 49 c fused multiply-adds.  With delta_0 = delta_2 = 0, r_max the largest 1 / deviation of the
 *   segment's channels, a_l = 2 delta_l + 765 u + 2^-40 and eps64 = 2^-45 max_ch (Q / N) / variance,
 *     |proj - exact| <= (1 + 1e-5) (r_max a_l sqrt(49 c) + (delta_l r_max + (49 c + 2) u / (1 - 49 c u) + eps64) sum_i |xhat_i w_i|)
 *   per entry, xhat the exactly normalised descriptor (derivation: the header of csrc/swd.hip; delta_l r_max <= 1e-3 assumed).
 * rcgan_sort_rows_f32: every row of x[rows][width] sorted ascending in place, in the total order of the keys
 *   bits ^ (sign ? 0xffffffff : 0x80000000): -0 before +0, +inf behind every finite value (the padding above relies on it).
 *   Bitonic: one launch for every compare-exchange stride below a chunk of min(width, 8192) floats held in LDS, one launch per
 *   stride at or above it; the kernel boundary is the only synchronisation between passes.  width 1: no launch.
 * rcgan_absdiff_rowsum: out[r] = sum_{i < count[r mod n_seg]} |a[r][i] - b[r][i]| in fp64 (a, b: [rows][width] fp32; count: int32
 *   DEVICE [n_seg], clamped to [0, width]), one workgroup per row, the order fixed by the launch geometry.
 * All four: on the context's stream, nothing written but the output (and `part`), no workspace, no host synchronisation, the same
 * bits on every run, legal inside a captured graph.
 * h, w each 28 or 32, c 1 or 3, level 0..2, stride >= 1 with n_pos <= 49, n >= 1, 1 <= n_seg <= 1024, 1 <= n_dir <= 1024, width a
 * power of two (sort: rows * width <= 2^36), rows >= 1, non-NULL pointers (x 16-byte, fp64 arrays 8-byte, the others 4-byte aligned):
 * anything else is RCGAN_EINVALID_ARG before any launch (a NULL context included, so the checks need no device). */
int rcgan_swd_moments(rcgan_ctx* ctx, int n, int h, int w, int c, int level, int stride, int n_seg, const uint8_t* x, const int32_t* off,
                      double* part, double* mom);
int rcgan_swd_project(rcgan_ctx* ctx, int n, int h, int w, int c, int level, int stride, int n_seg, const uint8_t* x, const int32_t* off,
                      const double* mom, int n_dir, const float* dirs, int width, float* proj);
int rcgan_sort_rows_f32(rcgan_ctx* ctx, int rows, int width, float* x);
int rcgan_absdiff_rowsum(rcgan_ctx* ctx, int rows, int width, int n_seg, const int32_t* count, const float* a, const float* b, double* out);

/* ---- azimuthally averaged power spectrum of square images (csrc/spectrum.hip; the radial power-spectrum distance of spectrum.py)
 * x: n images [n][N][N][c], NHWC, raw pixels 0..255 (uint8, DEVICE).  With a = x - 128 (exact),
 *   F_ch(u,v) = sum_{y,x} a[y][x][ch] exp(-2 pi i (u y + v x) / N),   P = |F|^2 / N^2,
 * signed frequencies f(u) = u if u <= N / 2 (integer division) else u - N, and the ring of (u,v) the integer b with
 *   (2b - 1)^2 <= 4 (f(u)^2 + f(v)^2) < (2b + 1)^2        (integer arithmetic; ring 0 is the point (0,0) alone),
 *   out[i][ch][b] = the mean of P over the members of ring b,   b < B(N) = 1 + the ring of (N/2, N/2)   (24 at 32, 21 at 28, 7 at 9).
 * Parseval: sum_b members_b out[i][ch][b] = sum a^2.  A smaller N is its own transform, not a zero-padded one.
 * Arithmetic: the transform in two passes of fp32 fused multiply-adds on the vector units, the twiddles computed in float64 on the
 * host (2 N values, passed as kernel arguments) and rounded to fp32; |F|^2, the ring sums (an order fixed by the launch geometry, no
 * floating-point atomics) and the mean in fp64, rounded once to fp32.  With u = 2^-24,
 *   |F^ - F| <= delta = g sum_{y,x} |a[y][x][ch]|,   g = sqrt(2) (2N + 8) u / (1 - (2N + 8) u),
 *   E = (2 mean_ring|F| delta + delta^2) / N^2,      |out - exact| <= E + 2 u (exact + E) + 2^-149
 * for every image, channel and ring (derivation: the header of csrc/spectrum.hip).  An image of 128s gives exact zeros.
 * One launch on the context's stream, every image's rings written on every call, nothing else written, no workspace, no host
 * synchronisation, the same bits on every run, legal inside a captured graph.
 * 8 <= N <= 32, c 1 or 3, n >= 1, non-NULL pointers (out 4-byte aligned; x of any alignment, 16-byte aligned images are read in
 * 16-byte loads): anything else is RCGAN_EINVALID_ARG before any launch (a NULL context included, so the checks need no device). */
int rcgan_radial_spectrum(rcgan_ctx* ctx, int n, int N, int c, const uint8_t* x, float* out /* [n][c][B(N)] */);

/* ---- optimiser ---------------------------------------------------------------------------------------- */
/* tf.train.AdamOptimizer on a flat fp32 range (model.py:250-262, gan_resnet.py:802-817):
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMA; w -= lr_t*m/(sqrt(v)+eps); optional clip to [-clip,clip]
 * (variable constraint of mnist/ops.py:102-111; clip<=0 disables).  hyper: DEVICE float[2] = {lr, t}
 * so a captured graph can be replayed with new values.  grad_scale multiplies g first (1/world_size). */
int rcgan_adam_tf(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v,
                  const float* hyper, float beta1, float beta2, float eps, float clip, float grad_scale);
/* The same with {lr, t} as launch arguments: an eagerly launched step (every optimiser step of both training loops: the
 * all-reduce sits between the captured graph and Adam) needs no host-to-device copy of two floats in front of it. */
int rcgan_adam_tf_host(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v,
                       float lr, float t, float beta1, float beta2, float eps, float clip, float grad_scale);
int rcgan_fill_f32(rcgan_ctx* ctx, size_t count, float* p, float value);
/* dst[i] = src[i] for `count` 4-byte words (both DEVICE-accessible), as a kernel on the context's stream: the hand-over of a step's
 * packed input batch (the feed_dict of gan_resnet.py:931,938) into the static input slab the captured step reads. */
int rcgan_copy_words(rcgan_ctx* ctx, size_t count, const void* src, void* dst);

/* ---- batch statistics out of the producing convolution (tf.nn.moments of normalization.py:47 fused into conv2d.py:181-216) ----------------
 * For the convolutions the 256 x 256 eight-wave kernel takes (rcgan_conv_stats_ok: 16-bit activations, Cout = 256, whole 256-pixel tiles,
 * the 32 x 32 generator block at n >= 50), rcgan_conv2d_fwd_stats is rcgan_conv2d_fwd_residual that also leaves, per pixel tile, the column
 * sums of the STORED output (bias, residual and the 16-bit rounding included) and of its squares in tile_sums (rcgan_conv_stats_bytes);
 * rcgan_bn_stats_from_tiles turns them into mean / rstd [nseg][Cout] of nseg equal runs of samples (biased variance, as rcgan_bn_stats):
 * the statistics pass over the activation tensor (one full read) disappears.  rcgan_bn_apply_segments: the apply half of
 * rcgan_bn_fwd_segments for statistics obtained that way (ws: nseg * rcgan_bn_workspace_bytes(n_per_seg*rows_per_sample, c), as there). */
int rcgan_conv_stats_ok(const rcgan_conv_desc* d);
size_t rcgan_conv_stats_bytes(const rcgan_conv_desc* d);
int rcgan_conv2d_fwd_stats(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias,
                           const void* residual, void* y, float* tile_sums);
int rcgan_bn_stats_from_tiles(rcgan_ctx* ctx, const rcgan_conv_desc* d, int nseg, float eps, const float* tile_sums, float* mean, float* rstd);
int rcgan_bn_apply_segments(rcgan_ctx* ctx, int nseg, int n_per_seg, int rows_per_sample, int c, int n_labels, int dtype, const void* x,
                            const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                            void* y, void* ws, size_t ws_bytes);

/* ---- gradient (loss) scaling for 16-bit activations ------------------------------------------------------------------------
 * The reference trains in fp32 (no counterpart in gan_resnet.py); BASELINE config 5 asks for fp16 activations, whose 5 exponent
 * bits need the loss -- hence every activation gradient -- scaled up.  rcgan_set_grad_scale: from now on every GRADIENT the loss
 * kernels emit (rcgan_loss_fwd_bwd, rcgan_bce_onehot_fwd_bwd, rcgan_proj_head_fwd_bwd) is multiplied by
 * host_scale * (*dev_scale if dev_scale != NULL); the loss VALUES they accumulate stay unscaled.  dev_scale is DEVICE memory read at
 * execution time, so a captured step follows a scale that changes between replays.  Default: 1, NULL. */
int rcgan_set_grad_scale(rcgan_ctx* ctx, float host_scale, const float* dev_scale);

/* ---- fp32 matmul precision (the counterpart of torch.set_float32_matmul_precision) -------------------------------------------
 * How the gather GEMM (conv_direct.hip: the fp32 convolutions, their data and filter gradients and the dense layers with fp32
 * activations) multiplies fp32 operands:
 *   RCGAN_F32_PRECISION_HIGHEST  v_mfma_f32_32x32x2_f32: exact fp32 products (default)
 *   RCGAN_F32_PRECISION_HIGH     every operand split into hi + lo bf16 (hi = bf16(x), lo = bf16(x - hi), nearest even) and
 *                                a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on v_mfma_f32_32x32x16_bf16, accumulated in fp32: about
 *                                16 significand bits per operand, error ~2^-16 * sum|a*b| on top of fp32 accumulation
 * The setting is read when a launch is ENQUEUED: a captured graph keeps the mode it was captured under.  Operands with 16-bit
 * activations and every other kernel (column sums, tiny / skinny dense layers, batch norm, spectral norm, Adam) are not affected.
 * Any other value: RCGAN_EINVALID_ARG. */
#define RCGAN_F32_PRECISION_HIGHEST 0
#define RCGAN_F32_PRECISION_HIGH 1
int rcgan_set_f32_matmul_precision(rcgan_ctx* ctx, int precision);
/* Dynamic loss scaling.  ls_state: DEVICE float[4] = {scale, applied steps since the last change, non-finite flag, skipped steps}.
 *   rcgan_grad_finite_check : raises the flag if g[0,count) holds an inf / nan (after the all-reduce: every rank sees the same sum);
 *   rcgan_adam_tf_dyn       : rcgan_adam_tf_host that (a) does nothing when the flag is raised (the step is skipped), (b) divides the
 *                             gradient by the current scale on top of grad_scale, (c) takes t = *t_dev + 1 (t_dev: DEVICE float[1],
 *                             the number of APPLIED updates of this group -- a skipped step does not advance the bias correction);
 *   rcgan_loss_scale_update : after the optimiser launches of a step: flag raised -> scale = max(scale/2, min_scale), flag cleared,
 *                             skipped++; else t_dev0 / t_dev1 (either may be NULL) += 1 and after growth_interval applied steps in
 *                             a row scale = min(2*scale, max_scale). */
int rcgan_grad_finite_check(rcgan_ctx* ctx, size_t count, const float* g, float* ls_state);
int rcgan_adam_tf_dyn(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v, float lr, const float* t_dev,
                      float beta1, float beta2, float eps, float clip, float grad_scale, const float* ls_state);
int rcgan_loss_scale_update(rcgan_ctx* ctx, float* ls_state, float* t_dev0, float* t_dev1, float growth_interval, float min_scale,
                            float max_scale);

/* ---- data-parallel gradient exchange (RCCL over xGMI) ------------------------------------------------------------------------
 * Replaces the reference's in-graph towers (cifar10/gan_resnet.py:529-546 tf.split over DEVICES, :697,786 tf.add_n(costs) / len(DEVICES)):
 * one process per GPU holds one tower; the gradients of the MEAN cost are the all-reduce SUM of the ranks' gradient buckets times
 * 1/world (applied by the optimiser kernel's grad_scale).  Every call is asynchronous on a stream and may be captured into the step's
 * hipGraph; RCGAN_ERCCL on any RCCL failure (rcgan_last_error carries ncclGetErrorString).
 *   rcgan_comm_unique_id       rank 0: 128 opaque bytes (ncclUniqueId) to hand to every rank (the host side moves them: file, TCP store, ...)
 *   rcgan_comm_init            collective over the `world` ranks: ncclCommInitRank on the context's device
 *   rcgan_comm_init_stub       single-process test double: "every rank holds what this rank holds", i.e. sum = world * x -- lets one GPU run
 *                              the whole world > 1 step schedule (buckets, side stream, in-graph optimiser) and compare it with world = 1
 *   rcgan_allreduce_sum        in place, fp32, on the context's stream
 *   rcgan_allreduce_sum_buckets  the same for several buckets as ONE RCCL group
 *   rcgan_allreduce_sum_async  on the communication stream, ordered after everything queued on the context's stream so far: the bucket must
 *                              be final; later launches of the backward pass run beside it (xGMI transfers under compute)
 *   rcgan_allreduce_join       the context's stream waits for the asynchronous buckets (before the optimiser reads them)
 *   rcgan_comm_count           the number of ranks the COMMUNICATOR reports (ncclCommCount; the test double: its world)
 *   rcgan_allreduce_sum_bf16_buckets  the same sum with the buckets travelling as bfloat16 (half the bytes over xGMI): every bucket is
 *                              rounded to bf16 (nearest even) into scratch16, summed there (ncclBfloat16) and widened back over the fp32 bucket,
 *                              three launches + one RCCL group whatever n.  scratch16: device memory, 2 bytes per float of all buckets together
 *                              (each bucket's part 256-byte aligned: rcgan_allreduce_bf16_scratch_bytes).  The sum of N bf16 values carries
 *                              8 mantissa bits: a gradient-precision trade the caller opts into
 *   rcgan_comm_stub_model      cost model of the test double: every all-reduce group then occupies its stream for
 *                              latency_us + 2 (world - 1) / world * bytes / bus_gbps (a one-thread kernel that watches the wall clock), so a
 *                              single GPU reports what a world-size-N step would take under a stated link model; 0, 0 = free */
#define RCGAN_COMM_ID_BYTES 128
int rcgan_comm_unique_id(void* id_out);
int rcgan_comm_init(rcgan_ctx* ctx, const void* id, int world, int rank);
int rcgan_comm_init_stub(rcgan_ctx* ctx, int world);
int rcgan_comm_destroy(rcgan_ctx* ctx);
int rcgan_comm_world(rcgan_ctx* ctx);
int rcgan_allreduce_sum(rcgan_ctx* ctx, float* buf, size_t count);
int rcgan_allreduce_sum_buckets(rcgan_ctx* ctx, int n, float* const* bufs, const size_t* counts);
int rcgan_allreduce_sum_async(rcgan_ctx* ctx, float* buf, size_t count);
int rcgan_allreduce_join(rcgan_ctx* ctx);
int rcgan_comm_count(rcgan_ctx* ctx, int* ranks);
size_t rcgan_allreduce_bf16_scratch_bytes(int n, const size_t* counts);
int rcgan_allreduce_sum_bf16_buckets(rcgan_ctx* ctx, int n, float* const* bufs, const size_t* counts, void* scratch16, size_t scratch_bytes);
int rcgan_comm_stub_model(rcgan_ctx* ctx, double bus_gbps, double latency_us);
/* why librccl could not be bound ("" when it was, or when nothing has tried yet) */
const char* rcgan_comm_load_error(void);
/* {a, b} -> p[0..1] by a one-thread launch on the stream: sets the DEVICE {lr, t} of rcgan_adam_tf in front of a replayed graph without a
 * host-to-device copy. */
int rcgan_set2_f32(rcgan_ctx* ctx, float* p, float a, float b);

/* ---- self test ---------------------------------------------------------------------------------------- */
/* Runs the MFMA / ds_read_b64_tr_b16 fragment-layout probes on the device (call once, outside graph
 * capture).  Fails iff the MFMA operand layout this library assumes does not hold; a failed
 * transpose-read probe only switches the filter-gradient kernel to its slower scalar LDS reads. */
int rcgan_selftest(rcgan_ctx* ctx);
#define RCGAN_QUERY_TR_READ 0   /* 1 = ds_read_b64_tr_b16 path in use, 0 = scalar fallback, -1 = not probed */
int rcgan_query(rcgan_ctx* ctx, int what);

#ifdef __cplusplus
}
#endif
#endif /* RCGAN_HIP_H */
