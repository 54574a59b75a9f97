// The matrix-core filter gradient (conv_wgrad.hip, conv_wgrad9.hip): argument block, planned problem, the kernels' order of precedence.
#pragma once
#include "conv_mfma.h"

struct ImgWGroup;   // conv_image.h

struct MfmaWgradArgs {
  const bf16_t* x;        // [N][H(/2)][W(/2)][Cin]
  const bf16_t* dy;       // [M][Cout]
  float* slab;            // [nz][slab_stride]: T*Cin*Cout filter-gradient partials (+ Cout bias-gradient partials)
  long slab_stride;       // floats between the slabs of two pixel chunks
  int want_bias;          // also emit column sums of dy (bias gradient) at slab[T*Cin*Cout ..]
  const bf16_t* zero;     // >= 16 zero bytes (halo / tail source of the direct-to-LDS loader)
  int N, H, W, Cin, Cout, KH, KW, PT, PL;
  int up, relu_in, use_tr;
  int lw, lh;
  long M, m_chunk;
  // Sub-pixel form of the filter gradient of an upsample-3x3 (sub = 1) or ConvMeanPool (sub = 2) layer, three-tap kernel only.
  // The reduction index runs over the LOW-resolution grid (N, H, W, lw, lh, M describe it; up = 0) and one operand is gathered
  // with stride 2 at a parity (pa, pb):
  //   sub 1: G[pa][pb][s][d] = sum_m x[n, i + dh, j + dw] * dy[n, 2i + pa, 2j + pb],   dh = s - 1 + pa, dw = d - 1 + pb
  //          (x = the stored low-resolution input, dy on the full-resolution grid)
  //   sub 2: G[pa][pb][s][d] = sum_m x[n, 2(i + dh) + pa, 2(j + dw) + pb] * dy[n, i, j],   dh = s - pa, dw = d - pb
  //          (x on the full-resolution grid, dy = the POOLED gradient; dW carries the pool's 1/4)
  // 16 matrices of Cin x Cout over M pixels instead of 9 over 4M: 4/9 of the multiply-adds.  The slab holds the 16 cells
  // [(pa*2 + pb)*4 + s*2 + d]; the slab reduction folds them into the 9 taps: dW[kh][kw] = scale * sum over the four parities of
  // G[pa][pb][S(pa, kh)][S(pb, kw)], S(sub 1) = {0: 0,1,1; 1: 0,0,1}, S(sub 2) = {0: 0,0,1; 1: 0,1,1}.
  //   sub 3: a small 1x1 filter (a down block's shortcut) on the two-tap body -- x and dy as they are, one tile row, the second
  //          tap idle: its filter gradient runs inside the grouped launch of the pass instead of a 16 us launch of its own
  int sub;
  int cells;              // filter cells per slab in front of the bias tail: KH*KW, or 16 in the sub-pixel form
};
// tile rows of the three-tap kernel's grid / multiply-adds per pixel and channel pair: reference formulation and executed
static inline int wgrad3_rows(const MfmaWgradArgs& a) { return a.sub == 3 ? 1 : (a.sub ? 8 : a.KH); }
static inline int wgrad3_alg_taps(const MfmaWgradArgs& a) { return a.sub == 3 ? 1 : (a.sub ? 36 : a.KH * a.KW); }
static inline int wgrad3_exec_taps(const MfmaWgradArgs& a) { return a.sub == 3 ? 1 : (a.sub ? 16 : a.KH * a.KW); }

// floats of one slab: the filter cells, then bias_tails rows of bias-gradient partials
static inline long wgrad_slab_floats(const MfmaWgradArgs& a, int bias_tails) { return (long)a.cells * a.Cin * a.Cout + (long)bias_tails * a.Cout; }
// a planned filter-gradient problem (mfma_wgrad_plan): gx tiles x gy pixel chunks of workgroups
struct MfmaWgradPlanned { MfmaWgradArgs a; unsigned gx, gy; };
// The four filter-gradient kernels in their order of precedence (mfma_wgrad_choose): all nine taps (sixteen sub-pixel cells) of a tile per
// workgroup (conv_wgrad9.hip); a filter row of three taps, the only home of the 1x1 form; one tap, direct-to-LDS; one tap, register-staged
// (single launches only).  WgradNine: the nine-tap kernel is on offer by the layer's own work (a launch alone), not at all, or wherever it
// takes the layer (a group decides for all its layers).  WGRAD*_ALONE_WGS: the workgroups a layer's launch alone aims at, per kernel.
enum WgradKernel { WK_NINE, WK_THREE, WK_TAP_GLDS, WK_TAP_REG };
enum WgradNine { WGRAD9_BY_WORK, WGRAD9_OFF, WGRAD9_ON };
constexpr int WGRAD_TAP_ALONE_WGS = 768, WGRAD3_ALONE_WGS = 512, WGRAD9_ALONE_WGS = 256;
// a filter gradient's workspace: nz slabs, then the column-sum partials of a bias gradient that the kernel leaves to colsum_launch
static inline size_t mfma_wgrad_ws_need(size_t nz, size_t slab_floats, long M, int cout) { return (nz * slab_floats + (size_t)((M + 2047) / 2048 + 1024) * cout) * sizeof(float); }

bool mfma_wgrad_eligible(const rcgan_conv_desc* d);
int mfma_wgrad_splits(const rcgan_conv_desc* d, long M, int sub);
size_t mfma_wgrad_ws_bytes(const rcgan_conv_desc* d);
int mfma_wgrad_sub_kind(const rcgan_conv_desc* d, int use_tr);
int mfma_wgrad_choose(rcgan_ctx* ctx, const MfmaWgradArgs& a, WgradNine nine, WgradKernel* k);
void mfma_wgrad_plan(MfmaWgradPlanned& p, WgradKernel k, int nz, long px_per_block);
#define WGRAD_GROUP_MAX 12        // problems per grouped launch of the three-tap / per-tap kernels (WgradGroup)
int mfma_wgrad3_group_launch(rcgan_ctx* ctx, int n, const MfmaWgradPlanned* probs, int family, const ImgWGroup* img, bool carry_head = false);
// conv_wgrad9.hip: all nine taps of a plain 3x3 layer in one workgroup (dy and x staged once for the three filter rows)
#define WGRAD9_GROUP_MAX 12
bool mfma_wgrad9_takes(const MfmaWgradArgs& a);
void mfma_wgrad9_plan(MfmaWgradPlanned& p, int nz, long px_per_block);      // mfma_wgrad_plan's nine-tap case
int mfma_wgrad9_group_launch(rcgan_ctx* ctx, int n, const MfmaWgradPlanned* probs);
int mfma_wgrad_launch(rcgan_ctx* ctx, MfmaWgradArgs& a, int nz, bool* bias_done, size_t ws_bytes);
// api.hip: the filter gradient of a layer the matrix cores do not take
int conv_wgrad_off_mfma(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                        void* ws, size_t ws_bytes);
