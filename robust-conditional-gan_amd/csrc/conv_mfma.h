// Argument block and declarations of the matrix-core forward / data-gradient convolution and of the filter preparation, shared by the
// conv_mfma*.hip kernels and api.hip (dispatch).  (The filter gradient's: conv_wgrad.h.)
#pragma once
#include "common.h"

struct ImgWArgs;    // conv_image.h

struct MfmaConvArgs {
  const bf16_t* in;       // [N][H(/2)][W(/2)][Cin]
  const bf16_t* wt;       // [Cout][T*Cin]
  const float* bias;      // [Cout] or null
  const bf16_t* mask;     // [M][Cout] or null: output zeroed where mask <= 0 (ReLU backward)
  const bf16_t* resid;    // [M][Cout] or null: added to the output (residual connection, gan_resnet.py:328)
  int resid_up;           // the residual lives on the HALF-resolution grid [N][H/2][W/2][Cout] and is added nearest-upsampled (lw, lh >= 1)
  bf16_t* out;            // [M][Cout]
  const bf16_t* zero;     // >= 16 zero bytes (halo source of the direct-to-LDS loader)
  int N, H, W, Cin, Cout, KH, KW, PT, PL;
  int up, relu_in, accumulate;
  int cm;                 // eight-wave kernels: channel-major K order (all taps of a 64-channel chunk, then the next chunk)
  int lw, lh;             // log2(W), log2(H) when both are powers of two (pixel decode by shifts), else -1
  long M;
  unsigned long long* stamps;   // diagnostics (rcgan_debug_stamps), normally null
  // Sub-pixel form of a 3x3 convolution behind the nearest 2x upsample (eight-wave kernels): output pixel (2i + ph, 2j + pw)
  // only sees the 2x2 source pixels (i + a - 1 + ph, j + b - 1 + pw), a, b in {0, 1}, each with the SUM of the filter taps that
  // fall on it -- four 2x2 convolutions over the low-resolution grid, 4/9 of the multiply-adds.  wph: the four summed filters
  // [phase = ph*2 + pw][Cout][(a*2 + b)*Cin + ci] (conv_prepare_phase_kernel), phase = 1: use them.  phase = 2: the data
  // gradient of that form, wph = [Cin][(u*4 + v)*Cout + co] (16 taps at source stride 2 over the full-resolution dy).
  const bf16_t* wph;
  int phase;              // MFMA_FORM_* below
  // eight-wave 256 x 256 kernel only: per-tile column sums of the stored output and of its squares, [pixel tile][Cout][2] fp32 --
  // the batch-norm statistics of the layer behind this convolution come out of its epilogue (bn.hip: bn_tile_stats_finish_kernel)
  float* stats;
  // halo-patch kernels (conv_mfma8h.hip) only: the input is act(cond_batch_norm(in)) -- the affine + ReLU of the batch norm IN FRONT of
  // this convolution applied to the staged patch in LDS, once per staged element, the normalised tensor never written (forward-only
  // passes: rcgan_conv2d_fwd_bn_residual).  mean / rstd [segments][Cin], gamma / beta [labels][Cin], labels [N] or null, bn_seg_samples
  // images per segment; bn_act RCGAN_ACT_NONE or RCGAN_ACT_RELU.  bn_mean == nullptr: off.
  const float* bn_mean = nullptr;
  const float* bn_rstd = nullptr;
  const float* bn_gamma = nullptr;
  const float* bn_beta = nullptr;
  const int32_t* bn_labels = nullptr;
  int bn_seg_samples = 1, bn_act = 0;
};

// MfmaConvArgs::phase.  (The kernels compare it with the literals.)
constexpr int MFMA_FORM_PLAIN = 0;      // KH x KW taps over the output grid; with `up` and `wph` the eight-wave / 64 x 64 kernels may still evaluate it sub-pixel
constexpr int MFMA_FORM_PHASE = 1;      // forced: four 2x2 convolutions over the low-resolution grid, filters = wph in the phase layout
constexpr int MFMA_FORM_GATHER = 2;     // forced: one 4x4 stride-2 convolution over the full-resolution grid, filters = wph in the gather layout

// The prepared buffer of a matrix-core layer, in 16-bit elements from its start (rcgan_conv_prepared_bytes sizes it, rcgan_conv_prepare /
// conv_prepare_batch_launch write it, api.hip's mfma_conv_pose reads it):
//   [0, T cin cout)              the forward layout [Cout][T*Cin]
//   [mfma_prepared_rot, ...)     the data gradient's: rotated taps, [Cin][T*Cout]
// and, where mfma_phase_filters(d), two blocks of 16 cin cout summed sub-pixel filters (conv_prepare_phase_kernel / prepare_phase_units
// get the first block's address and place the second themselves):
//   [mfma_prepared_sum_fwd, ...) the layer's FORWARD: phase layout of an upsample-3x3, gather layout of a ConvMeanPool
//   [mfma_prepared_sum_bwd, ...) its DATA GRADIENT: gather layout of an upsample-3x3, phase layout of a ConvMeanPool
static inline size_t mfma_prepared_rot(const rcgan_conv_desc* d) { return (size_t)d->kh * d->kw * d->cin * d->cout; }
static inline size_t mfma_prepared_sum_fwd(const rcgan_conv_desc* d) { return 2 * mfma_prepared_rot(d); }
static inline size_t mfma_prepared_sum_bwd(const rcgan_conv_desc* d) { return mfma_prepared_sum_fwd(d) + 16 * (size_t)d->cin * d->cout; }
static inline size_t mfma_prepared_sum_end(const rcgan_conv_desc* d) { return mfma_prepared_sum_bwd(d) + 16 * (size_t)d->cin * d->cout; }

static inline int ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

bool mfma_eligible(const rcgan_conv_desc* d);
bool mfma_phase_filters(const rcgan_conv_desc* d);
bool mfma_phase_dgrad_ok(const rcgan_conv_desc* d);
int conv_prepare_phase_launch(rcgan_ctx* ctx, int n, const float* const* ws, const float* const* sigmas, bf16_t* const* outs, const int* cins, const int* couts,
                              const int* kinds);
bool mfma_pool_ok(const rcgan_conv_desc* d);
int mfma_conv_launch(rcgan_ctx* ctx, const MfmaConvArgs& a);
int bn_tile_stats_finish_launch(rcgan_ctx* ctx, const float* part, int c, int nseg, int tiles_per_seg, int ngroups, long group_stride,
                                double count, float eps, float* mean, float* rstd);      // bn.hip
bool mfma_conv_is_p8(const MfmaConvArgs& a);              // routed to the 256 x 256 eight-wave kernel
bool mfma_conv8_phase_form(const MfmaConvArgs& a);        // ... which evaluates it in the sub-pixel (phase-major tile) form
int mfma_prepare_launch(rcgan_ctx* ctx, const float* w, const float* sigma, bf16_t* wt, bf16_t* wd, int T, int Cin, int Cout);
int direct_prepare_launch(rcgan_ctx* ctx, const float* w, const float* sigma, float* out, long total);
int mfma_selftest(rcgan_ctx* ctx, int* host_result);
// api.hip, for every translation unit that launches on the matrix cores: the one-off run of that self test (never inside a graph capture)
// and what it found about the transposing LDS read (-1 unknown, 0 no, 1 yes); the descriptor check of every convolution entry point
extern int g_use_tr;
int ensure_selftest(rcgan_ctx* ctx);
int check_desc(rcgan_ctx* ctx, const rcgan_conv_desc* d);
// image-end kernels (conv_image.hip): bf16 convs with a <= 3-channel side
int img_side(const rcgan_conv_desc* d);          // 0: not taken; 1: cin small; 2: cout small
size_t img_extra_offset(const rcgan_conv_desc* d);
size_t img_extra_bytes(const rcgan_conv_desc* d);
size_t img_wgrad_ws_bytes(const rcgan_conv_desc* d);
int img_prepare_launch(rcgan_ctx* ctx, const rcgan_conv_desc* d, const float* w, const float* sigma, void* prepared);
int img_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, void* y);
int img_dgrad(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* prepared, void* dx, int accumulate);
bool img_fwd_bn_ok(const rcgan_conv_desc* d);
int img_fwd_bn(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, void* y,
               const float* mean, const float* rstd, const float* gamma, const float* beta, const int32_t* labels, int segments, int act);
int img_wgrad_plan(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, int target_wgs, ImgWArgs* a, int* cb, int* nwg);
int img_wgrad(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
              void* ws, size_t ws_bytes);
int mfma_conv8_launch(rcgan_ctx* ctx, const MfmaConvArgs& a, bool wide, bool halo_patch);      // conv_mfma8.hip: 256 x 256 / 256 x 128 tiles, 8 wavefronts (halo_patch: conv_mfma8h.hip)
bool mfma_conv8_halo_takes(const MfmaConvArgs& a);                             // conv_mfma8h.hip: 256 x 256 tile, pixel operand as an LDS patch
int mfma_conv8_halo_launch(rcgan_ctx* ctx, const MfmaConvArgs& a);
bool mfma_conv8n_halo_takes(const MfmaConvArgs& a);                            // ... its 256 x 128-tile sibling (Cout % 128 == 0)
int mfma_conv8n_halo_launch(rcgan_ctx* ctx, const MfmaConvArgs& a);
int mfma_conv_bn_route(const MfmaConvArgs& a);                                 // would mfma_conv_launch run it on a halo-patch kernel?  1: 256 x 256, 2: 256 x 128, 0: no
struct SmallGemmArgs;
struct StepInputsArgs;
int conv_prepare_batch_launch(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n, const SmallGemmArgs* gemm = nullptr,
                              const StepInputsArgs* inputs = nullptr, const rcgan_frag_item* frags = nullptr, int n_frags = 0);
