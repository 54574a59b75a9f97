// extern "C" entry points: context, graphs, forward / data-gradient convolution and dense dispatch (MFMA vs direct), optimiser.
// (The filter gradient's entry points: conv_wgrad.hip.)
#include "conv_wgrad.h"
#include "small_gemm.h"
#include "step_inputs.h"
#include "conv_image.h"
#include "gather_plan.h"      // colsum_tail_bytes: the column-sum partials at the end of a transposed convolution's workspace

// ---- provided by the other translation units ------------------------------------------------------

size_t direct_wgrad_ws_bytes(const rcgan_conv_desc* d);
template <typename T> int direct_fwd(rcgan_ctx*, const rcgan_conv_desc*, const T*, const float*, const float*, const float*, T*, int n_cols = 0);
template <typename T> int direct_dgrad(rcgan_ctx*, const rcgan_conv_desc*, const T*, const float*, const float*, const float*, const T*, T*, int);
template <typename T> int direct_wgrad(rcgan_ctx*, const rcgan_conv_desc*, const T*, const T*, float*, float*, int, void*, size_t);
template <typename T> int direct_wgrad_cols(rcgan_ctx*, const rcgan_conv_desc*, const T*, const T*, int, const float*, float*, int, void*, size_t);
size_t direct_wgrad_cols_ws_bytes(const rcgan_conv_desc* d, int c1);
template <typename T> int colsum_launch(rcgan_ctx*, const T*, long, int, float*, int, float*);
template <typename T> int linear_fwd(rcgan_ctx*, long, long, long, const T*, const float*, const float*, const float*, T*);
template <typename T> int linear_dgrad(rcgan_ctx*, long, long, long, const T*, const float*, const float*, T*, int);
template <typename T> int linear_wgrad(rcgan_ctx*, long, long, long, const T*, const T*, float*, float*, int, void*, size_t);
size_t linear_wgrad_ws_bytes(long m, long k, long n);
template <typename T> int sumpool2_masked_launch(rcgan_ctx*, int, int, int, int, const T*, const T*, T*, int);
int small_fwd_kind(const rcgan_conv_desc* d);
int small_dgrad_kind(const rcgan_conv_desc* d);
int small_wgrad_kind(const rcgan_conv_desc* d);
size_t small_wgrad_ws_bytes(const rcgan_conv_desc* d);
template <typename T> int small_fwd(rcgan_ctx*, const rcgan_conv_desc*, int, const T*, const float*, const float*, T*);
template <typename T> int small_dgrad(rcgan_ctx*, const rcgan_conv_desc*, int, const T*, const float*, T*, int);
template <typename T> int small_wgrad(rcgan_ctx*, const rcgan_conv_desc*, int, const T*, const T*, float*, float*, int, void*, size_t);

// Dynamic loss scaling (fp16 activations).  ls: DEVICE float[4] = {scale, good steps since the last change, non-finite flag, skipped steps}.
// With ls the optimiser kernels (a) return without touching anything when the flag is set -- the step is skipped, (b) divide the
// gradient by the CURRENT scale on top of grad_scale, (c) take t = *tdev + 1 (tdev counts the APPLIED updates: a skipped step does
// not advance the bias correction).
struct AdamDyn { const float* ls; const float* tdev; };

__global__ void adam_tf_kernel(size_t count, float* w, const float* g, float* m, float* v, const float* hyper, float lr_v, float t_v,
                               float beta1, float beta2, float eps, float clip, float grad_scale, AdamDyn dyn) {
  if (dyn.ls) {
    if (dyn.ls[2] != 0.f) return;
    grad_scale /= dyn.ls[0];
    t_v = dyn.tdev[0] + 1.f;
  }
  // the arithmetic form of TF's ApplyAdam kernel: alpha = lr*sqrt(1-b2^t)/(1-b1^t);
  // m += (g-m)*(1-b1); v += (g*g-v)*(1-b2); w -= (m*alpha)/(sqrt(v)+eps), all in fp32
  // {lr, t}: device memory (a captured launch replayed with new values) or kernel arguments (hyper == nullptr)
  const float lr = hyper ? hyper[0] : lr_v, t = hyper ? hyper[1] : t_v;
  const float alpha = lr * sqrtf(1.f - powf(beta2, t)) / (1.f - powf(beta1, t));
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    float gi = g[i] * grad_scale;
    float mi = m[i] + (gi - m[i]) * omb1;
    float vi = v[i] + (gi * gi - v[i]) * omb2;
    float wi = w[i] - (mi * alpha) / (sqrtf(vi) + eps);
    if (clip > 0.f) wi = fminf(fmaxf(wi, -clip), clip);
    m[i] = mi; v[i] = vi; w[i] = wi;
  }
}

// the same update on four consecutive parameters per thread (16-byte accesses, one memory round trip per thread for slabs of up to
// 8M parameters): ranges whose start and length are multiples of four floats
__global__ void adam_tf_vec4_kernel(size_t count4, float4* w, const float4* g, float4* m, float4* v, const float* hyper, float lr_v, float t_v,
                                    float beta1, float beta2, float eps, float clip, float grad_scale, AdamDyn dyn) {
  if (dyn.ls) {
    if (dyn.ls[2] != 0.f) return;
    grad_scale /= dyn.ls[0];
    t_v = dyn.tdev[0] + 1.f;
  }
  const float lr = hyper ? hyper[0] : lr_v, t = hyper ? hyper[1] : t_v;
  const float alpha = lr * sqrtf(1.f - powf(beta2, t)) / (1.f - powf(beta1, t));
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 g4 = g[i], m4 = m[i], v4 = v[i], w4 = w[i];
    const float gs[4] = {g4.x, g4.y, g4.z, g4.w}, ms[4] = {m4.x, m4.y, m4.z, m4.w}, vs[4] = {v4.x, v4.y, v4.z, v4.w}, ws[4] = {w4.x, w4.y, w4.z, w4.w};
    float mo[4], vo[4], wo[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {      // (the operation sequence of adam_tf_kernel, element by element)
      const float gi = gs[q] * grad_scale;
      mo[q] = ms[q] + (gi - ms[q]) * omb1;
      vo[q] = vs[q] + (gi * gi - vs[q]) * omb2;
      wo[q] = ws[q] - (mo[q] * alpha) / (sqrtf(vo[q]) + eps);
      if (clip > 0.f) wo[q] = fminf(fmaxf(wo[q], -clip), clip);
    }
    m[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
    v[i] = make_float4(vo[0], vo[1], vo[2], vo[3]);
    w[i] = make_float4(wo[0], wo[1], wo[2], wo[3]);
  }
}

__global__ void set2_kernel(float* p, float a, float b) { p[0] = a; p[1] = b; }

// any non-finite value in g[0, count) raises the flag ls[2] (a benign race: every writer stores the same 1.0)
__global__ void grad_finite_check_kernel(size_t count, const float* g, float* ls) {
  bool bad = false;
  const size_t n4 = count / 4, stride = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n4; i += stride) {
    const float4 q = ((const float4*)g)[i];
    // x - x is 0 for finite x, NaN for +-inf and NaN
    const float z = (q.x - q.x) + (q.y - q.y) + (q.z - q.z) + (q.w - q.w);
    bad |= !(z == 0.f);
  }
  for (size_t i = n4 * 4 + tid; i < count; i += stride) bad |= !((g[i] - g[i]) == 0.f);
  if (bad) ls[2] = 1.f;
}

// one thread: skipped step -> halve the scale; applied step -> advance the groups' update counters, double the scale after
// `interval` applied steps in a row
__global__ void loss_scale_update_kernel(float* ls, float* t0, float* t1, float interval, float min_scale, float max_scale) {
  if (ls[2] != 0.f) {
    ls[0] = fmaxf(ls[0] * 0.5f, min_scale);
    ls[1] = 0.f; ls[2] = 0.f; ls[3] += 1.f;
  } else {
    if (t0) t0[0] += 1.f;
    if (t1) t1[0] += 1.f;
    ls[1] += 1.f;
    if (ls[1] >= interval) { if (ls[0] < max_scale) ls[0] = fminf(ls[0] * 2.f, max_scale); ls[1] = 0.f; }
  }
}

static void adam_launch(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v, const float* hyper, float lr, float t,
                        float beta1, float beta2, float eps, float clip, float grad_scale, AdamDyn dyn = {nullptr, nullptr}) {
  const bool vec = count % 4 == 0 && (((size_t)w | (size_t)g | (size_t)m | (size_t)v) & 15) == 0;
  if (vec) {
    size_t blocks = (count / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(adam_tf_vec4_kernel, dim3((int)blocks), dim3(256), 0, ctx->stream, count / 4, (float4*)w, (const float4*)g, (float4*)m,
                       (float4*)v, hyper, lr, t, beta1, beta2, eps, clip, grad_scale, dyn);
  } else {
    size_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adam_tf_kernel, dim3((int)blocks), dim3(256), 0, ctx->stream, count, w, g, m, v, hyper, lr, t, beta1, beta2, eps, clip,
                       grad_scale, dyn);
  }
}

int g_use_tr = -1;   // -1 unknown, 0 no, 1 yes (decided by the self test)

int ensure_selftest(rcgan_ctx* ctx) {
  if (g_use_tr >= 0) return RCGAN_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(ctx->stream, &st);
  if (st != hipStreamCaptureStatusNone) RC_FAIL(ctx, RCGAN_EINVALID_ARG, "first MFMA wgrad call must happen outside graph capture");
  int res[2] = {0, 0};
  int rc = mfma_selftest(ctx, res);
  if (rc) return rc;
  if (res[0] != 0) RC_FAIL(ctx, RCGAN_EHIP, "MFMA 16x16x32 bf16 fragment layout probe failed (%d mismatches)", res[0]);
  g_use_tr = (res[1] == 0) ? 1 : 0;
  const char* e = getenv("RCGAN_NO_TR");
  if (e && e[0] == '1') g_use_tr = 0;
  return RCGAN_OK;
}

int check_desc(rcgan_ctx* ctx, const rcgan_conv_desc* d) {
  RC_REQUIRE(ctx, d != nullptr, "null desc");
  RC_REQUIRE(ctx, d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0, "bad dims");
  RC_REQUIRE(ctx, d->kh > 0 && d->kw > 0 && d->stride > 0, "bad kernel/stride");
  RC_REQUIRE(ctx, d->dtype == RCGAN_F32 || d->dtype == RCGAN_H16, "bad dtype");
  if (d->flags & RCGAN_CONV_IN_UPSAMPLE2X) RC_REQUIRE(ctx, d->h % 2 == 0 && d->w % 2 == 0, "upsampled size must be even");
  if (d->flags & RCGAN_CONV_OUT_MEANPOOL2)
    RC_REQUIRE(ctx, !(d->flags & RCGAN_CONV_IN_UPSAMPLE2X) && d->h % 2 == 0 && d->w % 2 == 0, "fused mean pool: even size, no upsampled input");
  return RCGAN_OK;
}

// The filter gradient of a layer the matrix cores do not take (rcgan_conv2d_bwd_weight, conv_wgrad.hip): image-end, small or direct kernel
int conv_wgrad_off_mfma(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                        void* ws, size_t ws_bytes) {
  if (img_side(d)) return img_wgrad(ctx, d, x, dy, dw, dbias, accumulate, ws, ws_bytes);
  if (int kind = small_wgrad_kind(d)) {
    RC_DISPATCH_DTYPE(ctx, d->dtype, return small_wgrad<T>(ctx, d, kind, (const T*)x, (const T*)dy, dw, dbias, accumulate, ws, ws_bytes));
  }
  RC_DISPATCH_DTYPE(ctx, d->dtype, return direct_wgrad<T>(ctx, d, (const T*)x, (const T*)dy, dw, dbias, accumulate, ws, ws_bytes));
  return RCGAN_OK;
}

extern "C" {

const char* rcgan_version(void) { return RCGAN_HALF_FP16 ? "rcgan_hip 0.1 (gfx950, fp16 build)" : "rcgan_hip 0.1 (gfx950, bf16 build)"; }

int rcgan_create(rcgan_ctx** out, int device, void* stream) {
  if (!out) return RCGAN_EINVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return RCGAN_EHIP;
  if (hipSetDevice(device) != hipSuccess) return RCGAN_EHIP;
  rcgan_ctx* c = new rcgan_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  c->capturing = false;
  c->devtmp = nullptr;
  c->devtmp_bytes = 0;
  c->prof_which = 0;
  c->prof_flops = 0.0; c->prof_flops_exec = 0.0;
  c->main_stream = c->stream; c->side_stream = nullptr; c->fork_ev = nullptr; c->join_ev = nullptr; c->on_side = false;
  if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return RCGAN_EHIP;
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    c->num_cus = cus;
  }
  c->dbg_stamps = nullptr;
  c->head_stage = 0;
  c->comm = nullptr; c->comm_world = 1; c->comm_rank = 0; c->comm_stub = false; c->comm_stream = nullptr;
  c->comm_fork = nullptr; c->comm_join = nullptr; c->comm_pending = false;
  c->stub_bus_gbps = 0.0; c->stub_latency_us = 0.0; c->wall_clock_khz = 0;
  c->narrow_ws = nullptr; c->narrow_ws_bytes = 0; c->splitr_ws = nullptr; c->splitr_ws_bytes = 0;
  c->gscale_host = 1.f;
  c->gscale_dev = nullptr;
  c->f32_precision = RCGAN_F32_PRECISION_HIGHEST;
  c->zero_page = nullptr;
  if (hipMalloc(&c->zero_page, RC_ZERO_PAGE_BYTES) != hipSuccess || hipMemset(c->zero_page, 0, RC_ZERO_PAGE_BYTES) != hipSuccess) {
    delete c;
    return RCGAN_EHIP;
  }
  for (int i = 0; i < 64; ++i) c->event_made[i] = false;
  *out = c;
  return RCGAN_OK;
}

int rcgan_destroy(rcgan_ctx* ctx) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  (void)hipStreamSynchronize(ctx->stream);
  // graphs first: captured ncclAllReduce nodes hold references to the communicator, which RCCL wants released before ncclCommDestroy
  for (auto& g : ctx->graphs)
    if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
  (void)rcgan_comm_destroy(ctx);
  for (int i = 0; i < 64; ++i)
    if (ctx->event_made[i]) (void)hipEventDestroy(ctx->events[i]);
  if (ctx->zero_page) (void)hipFree(ctx->zero_page);
  if (ctx->narrow_ws) (void)hipFree(ctx->narrow_ws);
  if (ctx->splitr_ws) (void)hipFree(ctx->splitr_ws);
  for (void* p : ctx->retired_ws) (void)hipFree(p);
  if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
  if (ctx->join_ev) (void)hipEventDestroy(ctx->join_ev);
  if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
  delete ctx;
  return RCGAN_OK;
}

const char* rcgan_last_error(rcgan_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }
int rcgan_half_dtype(void) { return RCGAN_H16; }

// CRC-32C, slice-by-8 tables built on first use (host only)
unsigned rcgan_crc32c(unsigned crc, const void* data, size_t n) {
  static uint32_t tab[8][256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      tab[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int t = 1; t < 8; ++t) tab[t][i] = (tab[t - 1][i] >> 8) ^ tab[0][tab[t - 1][i] & 0xff];
    ready = true;
  }
  const unsigned char* p = (const unsigned char*)data;
  uint32_t c = ~crc;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = tab[7][lo & 0xff] ^ tab[6][(lo >> 8) & 0xff] ^ tab[5][(lo >> 16) & 0xff] ^ tab[4][lo >> 24] ^
        tab[3][hi & 0xff] ^ tab[2][(hi >> 8) & 0xff] ^ tab[1][(hi >> 16) & 0xff] ^ tab[0][hi >> 24];
    p += 8; n -= 8;
  }
  while (n--) c = (c >> 8) ^ tab[0][(c ^ *p++) & 0xff];
  return ~c;
}

int rcgan_set_stream(rcgan_ctx* ctx, void* stream) {
  RC_REQUIRE(ctx, !ctx->on_side, "set_stream inside a side section");
  ctx->stream = ctx->main_stream = (hipStream_t)stream;
  return RCGAN_OK;
}

// Fork: launches issued until rcgan_side_end go to the side stream, ordered after everything issued so far on the main
// stream.  Join: the main stream waits for the side section.  Between end and join the two streams run concurrently.
int rcgan_side_begin(rcgan_ctx* ctx) {
  RC_REQUIRE(ctx, !ctx->on_side, "side sections do not nest");
  RC_HIP(ctx, hipEventRecord(ctx->fork_ev, ctx->main_stream));
  RC_HIP(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->fork_ev, 0));
  ctx->stream = ctx->side_stream;
  ctx->on_side = true;
  return RCGAN_OK;
}

int rcgan_side_end(rcgan_ctx* ctx) {
  RC_REQUIRE(ctx, ctx->on_side, "no side section open");
  RC_HIP(ctx, hipEventRecord(ctx->join_ev, ctx->side_stream));
  ctx->stream = ctx->main_stream;
  ctx->on_side = false;
  return RCGAN_OK;
}

int rcgan_side_join(rcgan_ctx* ctx) {
  RC_REQUIRE(ctx, !ctx->on_side, "close the side section first");
  RC_HIP(ctx, hipStreamWaitEvent(ctx->main_stream, ctx->join_ev, 0));
  return RCGAN_OK;
}

int rcgan_stream_sync(rcgan_ctx* ctx) {
  RC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RCGAN_OK;
}

int rcgan_event_record(rcgan_ctx* ctx, int slot) {
  RC_REQUIRE(ctx, slot >= 0 && slot < 64, "slot %d", slot);
  if (!ctx->event_made[slot]) {
    RC_HIP(ctx, hipEventCreate(&ctx->events[slot]));
    ctx->event_made[slot] = true;
  }
  RC_HIP(ctx, hipEventRecord(ctx->events[slot], ctx->stream));
  return RCGAN_OK;
}

int rcgan_event_elapsed_ms(rcgan_ctx* ctx, int s0, int s1, float* ms) {
  RC_REQUIRE(ctx, s0 >= 0 && s0 < 64 && s1 >= 0 && s1 < 64 && ctx->event_made[s0] && ctx->event_made[s1], "bad slots");
  RC_HIP(ctx, hipEventSynchronize(ctx->events[s1]));
  RC_HIP(ctx, hipEventElapsedTime(ms, ctx->events[s0], ctx->events[s1]));
  return RCGAN_OK;
}

int rcgan_graph_begin(rcgan_ctx* ctx) {
  RC_REQUIRE(ctx, !ctx->capturing, "already capturing");
  RC_REQUIRE(ctx, ctx->stream != nullptr, "graph capture needs a non-null stream");
  RC_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  ctx->capturing = true;
  return RCGAN_OK;
}

int rcgan_reserve_scratch(rcgan_ctx* ctx, size_t bytes) {
  RC_REQUIRE(ctx, !ctx->capturing, "scratch cannot grow inside a capture");
  RC_HIP(ctx, ctx_grow_scratch(ctx, &ctx->splitr_ws, &ctx->splitr_ws_bytes, bytes));
  RC_HIP(ctx, ctx_grow_scratch(ctx, &ctx->narrow_ws, &ctx->narrow_ws_bytes, bytes));
  return RCGAN_OK;
}

int rcgan_scratch_bytes(rcgan_ctx* ctx, size_t* split_reduction_bytes, size_t* narrow_bytes) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  if (split_reduction_bytes) *split_reduction_bytes = ctx->splitr_ws_bytes;
  if (narrow_bytes) *narrow_bytes = ctx->narrow_ws_bytes;
  return RCGAN_OK;
}

int rcgan_graph_end(rcgan_ctx* ctx, int* graph_id) {
  RC_REQUIRE(ctx, ctx->capturing, "not capturing");
  hipGraph_t g = nullptr;
  ctx->capturing = false;
  RC_HIP(ctx, hipStreamEndCapture(ctx->stream, &g));
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) RC_FAIL(ctx, RCGAN_EHIP, "hipGraphInstantiate -> %s", hipGetErrorString(e));
  ctx->graphs.push_back(ge);
  *graph_id = (int)ctx->graphs.size() - 1;
  return RCGAN_OK;
}

int rcgan_graph_abort(rcgan_ctx* ctx) {
  // Leave a capture that cannot be completed (a launch inside it failed): what was recorded is dropped, nothing was executed.
  if (!ctx) return RCGAN_EINVALID_ARG;
  if (!ctx->capturing) return RCGAN_OK;
  ctx->capturing = false;
  ctx->head_stage = 0;           // (deferred launches recorded into the dropped capture never ran; their buffers belong to the aborted step)
  ctx->comm_pending = false;     // (an asynchronous bucket's join event was recorded inside the dropped capture)
  hipGraph_t g = nullptr;
  (void)hipStreamEndCapture(ctx->stream, &g);
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  return RCGAN_OK;
}

int rcgan_graph_launch(rcgan_ctx* ctx, int id) {
  RC_REQUIRE(ctx, id >= 0 && id < (int)ctx->graphs.size() && ctx->graphs[id], "graph id %d", id);
  RC_HIP(ctx, hipGraphLaunch(ctx->graphs[id], ctx->stream));
  return RCGAN_OK;
}

int rcgan_graph_destroy(rcgan_ctx* ctx, int id) {
  RC_REQUIRE(ctx, id >= 0 && id < (int)ctx->graphs.size() && ctx->graphs[id], "graph id %d", id);
  (void)hipGraphExecDestroy(ctx->graphs[id]);
  ctx->graphs[id] = nullptr;
  return RCGAN_OK;
}

int rcgan_set_f32_matmul_precision(rcgan_ctx* ctx, int precision) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  RC_REQUIRE(ctx, precision == RCGAN_F32_PRECISION_HIGHEST || precision == RCGAN_F32_PRECISION_HIGH, "fp32 matmul precision %d", precision);
  ctx->f32_precision = precision;
  return RCGAN_OK;
}

int rcgan_debug_stamps(rcgan_ctx* ctx, void* stamps) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  ctx->dbg_stamps = stamps;
  return RCGAN_OK;
}

int rcgan_prof_begin(rcgan_ctx* ctx, int which) {
  for (auto e : ctx->prof_ev) (void)hipEventDestroy(e);
  ctx->prof_ev.clear();
  ctx->prof_flops = 0.0;
  ctx->prof_flops_exec = 0.0;
  ctx->prof_bn_in = 0;
  ctx->prof_which = which;
  return RCGAN_OK;
}

int rcgan_prof_end(rcgan_ctx* ctx, int* launches, double* total_ms, double* total_flops) {
  ctx->prof_which = 0;
  RC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double ms = 0.0;
  size_t n = ctx->prof_ev.size() / 2;
  for (size_t i = 0; i < n; ++i) {
    float t = 0.f;
    RC_HIP(ctx, hipEventElapsedTime(&t, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
    ms += t;
  }
  for (auto e : ctx->prof_ev) (void)hipEventDestroy(e);
  ctx->prof_ev.clear();
  if (launches) *launches = (int)n;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = ctx->prof_flops;
  return RCGAN_OK;
}

int rcgan_prof_executed_flops(rcgan_ctx* ctx, double* executed_flops) {
  RC_REQUIRE(ctx, executed_flops != nullptr, "null argument");
  *executed_flops = ctx->prof_flops_exec;
  return RCGAN_OK;
}

int rcgan_prof_bn_in_launches(rcgan_ctx* ctx, int* launches) {
  if (!ctx || !launches) return RCGAN_EINVALID_ARG;
  *launches = ctx->prof_bn_in;
  return RCGAN_OK;
}

int rcgan_selftest(rcgan_ctx* ctx) {
  g_use_tr = -1;
  return ensure_selftest(ctx);
}

int rcgan_query(rcgan_ctx* ctx, int what) {
  (void)ctx;
  if (what == RCGAN_QUERY_TR_READ) return g_use_tr;
  return RCGAN_EINVALID_ARG;
}

// ------------------------------------------------------------------------------------------------
// convolution
// ------------------------------------------------------------------------------------------------
int rcgan_conv_fused_pool_ok(const rcgan_conv_desc* d) { return d && mfma_pool_ok(d) ? 1 : 0; }

size_t rcgan_conv_prepared_bytes(const rcgan_conv_desc* d) {
  size_t elems = (size_t)d->kh * d->kw * d->cin * d->cout;
  if (mfma_eligible(d)) return (mfma_phase_filters(d) ? mfma_prepared_sum_end(d) : mfma_prepared_sum_fwd(d)) * sizeof(bf16_t) + 256;
  if (img_side(d)) return img_extra_offset(d) + img_extra_bytes(d);
  return elems * sizeof(float) + 256;
}

int rcgan_conv_prepare(rcgan_ctx* ctx, const rcgan_conv_desc* d, const float* w, const float* sigma, void* prepared) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  const int T = d->kh * d->kw;
  size_t elems = (size_t)T * d->cin * d->cout;
  if (mfma_eligible(d)) {
    bf16_t* wt = (bf16_t*)prepared;
    rc = mfma_prepare_launch(ctx, w, sigma, wt, wt + mfma_prepared_rot(d), T, d->cin, d->cout);
    if (rc || !mfma_phase_filters(d)) return rc;
    bf16_t* wph = wt + mfma_prepared_sum_fwd(d);
    const int kind = (d->flags & RCGAN_CONV_OUT_MEANPOOL2) ? 1 : 0;
    return conv_prepare_phase_launch(ctx, 1, &w, &sigma, &wph, &d->cin, &d->cout, &kind);
  }
  rc = direct_prepare_launch(ctx, w, sigma, (float*)prepared, (long)elems);
  if (rc) return rc;
  return img_prepare_launch(ctx, d, w, sigma, prepared);
}

int rcgan_conv_prepare_batch(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items) {
  RC_REQUIRE(ctx, items != nullptr && n_items >= 0, "bad items");
  for (int i = 0; i < n_items; ++i) {
    int rc = check_desc(ctx, &items[i].desc);
    if (rc) return rc;
  }
  return conv_prepare_batch_launch(ctx, items, n_items);
}

int rcgan_conv_prepare_batch_embed(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e) {
  return rcgan_conv_prepare_batch_riders(ctx, items, n_items, e, nullptr);
}

int rcgan_conv_prepare_batch_riders(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e,
                                    const rcgan_step_inputs_desc* si) {
  return rcgan_conv_prepare_batch_frags(ctx, items, n_items, e, si, nullptr, 0);
}

int rcgan_conv_prepare_batch_frags(rcgan_ctx* ctx, const rcgan_prepare_item* items, int n_items, const rcgan_embed_desc* e,
                                   const rcgan_step_inputs_desc* si, const rcgan_frag_item* frags, int n_frags) {
  if (e == nullptr && si == nullptr && n_frags == 0) return rcgan_conv_prepare_batch(ctx, items, n_items);
  RC_REQUIRE(ctx, items != nullptr && n_items >= 1, "the riders need at least one filter to ride with");
  RC_REQUIRE(ctx, n_frags >= 0 && n_frags <= 12 && (n_frags == 0 || frags != nullptr), "%d fragment copies (at most 12)", n_frags);
  for (int f = 0; f < n_frags; ++f) {
    RC_REQUIRE(ctx, frags[f].item >= 0 && frags[f].item < n_items && frags[f].fwd && frags[f].bwd, "fragment copy %d: bad item / null destination", f);
    const rcgan_conv_desc& d = items[frags[f].item].desc;
    RC_REQUIRE(ctx, mfma_eligible(&d) && d.kh == 3 && d.kw == 3 && frags[f].ctn >= 1 && frags[f].ss >= 1 && d.cout % (16 * frags[f].ctn) == 0 &&
                        d.cin % (16 * frags[f].ctn) == 0 && (9 * d.cin / 32) % frags[f].ss == 0 && (9 * d.cout / 32) % frags[f].ss == 0,
               "fragment copy %d: not a 16-bit 3x3 filter this layout divides (%d -> %d, %d tiles, %d steps)", f, d.cin, d.cout, frags[f].ctn, frags[f].ss);
  }
  for (int i = 0; i < n_items; ++i) {
    int rc = check_desc(ctx, &items[i].desc);
    if (rc) return rc;
  }
  SmallGemmArgs ge;
  if (e) {
    RC_REQUIRE(ctx, e->v >= 1 && e->v <= HEAD_MAX_V && e->e_dim >= 1 && e->d >= 1 && e->table && e->w_e && e->E, "bad embed desc");
    // E[l][j] = (sum_k table[l][k] W_e[k][j]) / sigma_e + b_e[j]   (the first small-left GEMM of rcgan_proj_head_fwd_bwd)
    ge = {e->v, e->e_dim, e->d, e->table, e->e_dim, 1, e->w_e, e->sigma_e, e->b_e, e->E, nullptr, 0};
  }
  StepInputsArgs sa;
  if (si) {
    RC_REQUIRE(ctx, si->n >= 1 && si->images && si->x && si->rng_state, "bad step-inputs desc");
    RC_REQUIRE(ctx, si->dtype == RCGAN_F32 || si->dtype == RCGAN_H16, "bad dtype");
    RC_REQUIRE(ctx, si->fill == nullptr || (si->fill_count % 4 == 0 && ((size_t)si->fill & 15) == 0), "fill range must be whole float4");
    sa.n = si->n; sa.is16 = si->dtype == RCGAN_H16 ? 1 : 0; sa.img = si->images; sa.x = si->x; sa.pooled = si->pooled;
    sa.lo = si->noise_lo; sa.hi = si->noise_hi; sa.seed = si->seed; sa.state = (uint64_t*)si->rng_state;
    sa.counter = ctx->counters() + RC_COUNTER_INPUTS;
    sa.fill = si->fill; sa.fill4 = si->fill ? si->fill_count / 4 : 0;
    sa.fakes = si->fakes; sa.slice = (unsigned*)si->fake_slice; sa.nslices = si->n_slices;
    RC_REQUIRE(ctx, si->fakes == nullptr || (si->fake_slice != nullptr && si->n_slices >= 1 && ((size_t)si->fakes & 15) == 0 && ((size_t)si->x & 15) == 0),
               "fake slices need a device counter and 16-byte aligned tensors");
  }
  return conv_prepare_batch_launch(ctx, items, n_items, e ? &ge : nullptr, si ? &sa : nullptr, frags, n_frags);
}

size_t rcgan_conv_workspace_bytes(const rcgan_conv_desc* d) {
  size_t ws = direct_wgrad_ws_bytes(d);
  if (small_wgrad_kind(d)) {
    size_t s = small_wgrad_ws_bytes(d);
    if (s > ws) ws = s;
  }
  if (img_side(d)) {
    size_t s = img_wgrad_ws_bytes(d);
    if (s > ws) ws = s;
  }
  if (mfma_wgrad_eligible(d)) ws = std::max(ws, mfma_wgrad_ws_bytes(d));
  // upsample-folded data gradient: full-resolution dx scratch
  if (d->flags & RCGAN_CONV_IN_UPSAMPLE2X) {
    size_t s = (size_t)d->n * d->h * d->w * d->cin * dtype_size(d->dtype) + 256;
    if (s > ws) ws = s;
  }
  return ws;
}

// RCGAN_CONV_RESID_UPSAMPLE2X: the matrix-core epilogue reads the half-resolution residual in place (power-of-two output grid)
int rcgan_conv_resid_up_ok(const rcgan_conv_desc* d) {
  return d && mfma_eligible(d) && !(d->flags & RCGAN_CONV_OUT_MEANPOOL2) && d->stride == 1 && ilog2_exact(d->w) >= 1 && ilog2_exact(d->h) >= 1 ? 1 : 0;
}

// ---- posing a matrix-core launch ----------------------------------------------------------------------------------------------
// THE translation of a descriptor into the MfmaConvArgs that mfma_conv_route routes and mfma_conv_launch issues: which of the six forms
// (plain / phase / gather, forward or data gradient) the layer runs in, which filter layout of the prepared buffer (conv_mfma.h:
// mfma_prepared_*) the kernel reads, and the guards in front of every launch.  The entry points add the fields their fused form owns
// (stats, bn_*, resid, mask); the routing queries pose with ctx == nullptr and null tensors and ask the routing about the same struct.
enum ConvDir { CONV_FWD, CONV_DGRAD };

// Queries have no zero page and no prepared buffer, and the routing only asks whether they are THERE (mfma_conv_route: a.zero != nullptr;
// mfma_conv8_phase_form: a.wph != nullptr) -- nothing is read through this stand-in.
static const bf16_t pose_query_stand_in[8] = {0};

// in / out: x / y (forward), dy / dx (data gradient).  has_resid: a residual tensor will be added by the epilogue.
static int mfma_conv_pose(rcgan_ctx* ctx, const rcgan_conv_desc* d, ConvDir dir, const void* in, const void* prepared, const float* bias,
                          bool has_resid, void* out, MfmaConvArgs* posed) {
  auto fail = [&](int code, const char* what) { if (ctx) ctx->err = std::string("mfma_conv_pose: ") + what; return code; };
  *posed = MfmaConvArgs{};      // (value-initialised whatever follows: a routing question never reads an indeterminate field)
  MfmaConvArgs& a = *posed;
  const bool query = ctx == nullptr;
  const bool pool = d->flags & RCGAN_CONV_OUT_MEANPOOL2, up = d->flags & RCGAN_CONV_IN_UPSAMPLE2X;
  if (pool && !(rcgan_conv_fused_pool_ok(d) && !has_resid))
    return fail(RCGAN_EINVALID_ARG, "fused mean pool not available for this convolution (rcgan_conv_fused_pool_ok)");
  if (!mfma_eligible(d)) return fail(RCGAN_EUNSUPPORTED_SHAPE, "not a matrix-core convolution");
  if ((long)d->n * d->h * d->w * (d->cin > d->cout ? d->cin : d->cout) >= (1L << 31))
    return fail(RCGAN_EUNSUPPORTED_SHAPE, "tensor exceeds the 32-bit element offsets of the MFMA kernels");
  int oh, ow;
  same_pad(d->h, d->kh, 1, &oh, &a.PT);
  same_pad(d->w, d->kw, 1, &ow, &a.PL);
  a.N = d->n; a.H = d->h; a.W = d->w; a.KH = d->kh; a.KW = d->kw;
  a.M = (long)d->n * d->h * d->w;
  const long m_low = (long)d->n * (d->h / 2) * (d->w / 2);      // the gather forms run over the low-resolution grid
  a.lw = ilog2_exact(d->w); a.lh = ilog2_exact(d->h);
  if (a.lw < 0 || a.lh < 0) { a.lw = -1; a.lh = -1; }
  a.in = (const bf16_t*)in; a.bias = bias; a.out = (bf16_t*)out;
  a.zero = query ? pose_query_stand_in : (const bf16_t*)ctx->zero_page;
  a.accumulate = (d->flags & RCGAN_CONV_ACCUMULATE) ? 1 : 0;
  auto filters = [&](size_t at) { return query ? pose_query_stand_in : (const bf16_t*)prepared + at; };
  if (dir == CONV_FWD) {
    a.wt = filters(0);
    a.Cin = d->cin; a.Cout = d->cout;
    a.relu_in = (d->flags & RCGAN_CONV_IN_RELU) ? 1 : 0;
    if (pool) {
      // ConvMeanPool as one 4x4 stride-2 convolution over x (16 taps, summed filters x 1/4): y over the pooled grid
      a.M = m_low;
      a.wph = filters(mfma_prepared_sum_fwd(d));        // gather layout [Cout][16 * Cin]
      a.phase = MFMA_FORM_GATHER;
    } else {
      // an upsample-3x3 takes its summed filters [4][Cout][4 * Cin] along and stays MFMA_FORM_PLAIN: the routing runs it sub-pixel where
      // whole tiles fall into one phase (mfma_conv8_phase_form, launch_conv_mfma), else over floor(row / 2) sources with wt
      a.up = up ? 1 : 0;
      if (up && mfma_phase_filters(d)) a.wph = filters(mfma_prepared_sum_fwd(d));
      a.resid_up = (has_resid && (d->flags & RCGAN_CONV_RESID_UPSAMPLE2X)) ? 1 : 0;
      if (a.resid_up && !rcgan_conv_resid_up_ok(d))
        return fail(RCGAN_EINVALID_ARG, "half-resolution residual not available for this convolution (rcgan_conv_resid_up_ok)");
    }
  } else {
    a.Cin = d->cout; a.Cout = d->cin;          // reduction over cout, output channels = cin
    if (pool) {
      // dy lives on the pooled grid: dx (full resolution) in the sub-pixel form -- pixel (2i + ph, 2j + pw) gathers the 2x2 pooled
      // pixels around it with the transposed summed filters of its phase
      a.wt = filters(0);                                    // (not a usable fallback: mfma_conv_route never leaves the phase form)
      a.up = 1;                                             // source grid = the pooled one (h/2 x w/2)
      a.wph = filters(mfma_prepared_sum_bwd(d));            // phase layout [4][Cin][4 * Cout]
      a.phase = MFMA_FORM_PHASE;
    } else if (up && mfma_phase_dgrad_ok(d)) {
      // sub-pixel form: dx over the low-resolution grid straight from dy (16 taps at stride 2, transposed summed filters), the
      // ReLU mask and the accumulation in the epilogue -- no full-resolution scratch, no 2x2 sum pass
      a.wt = filters(mfma_prepared_rot(d));
      a.M = m_low;
      a.wph = filters(mfma_prepared_sum_bwd(d));            // gather layout [Cin][16 * Cout]
      a.phase = MFMA_FORM_GATHER;
    } else {
      // rotated filters, mirrored padding.  Behind an upsample this is dx on the FULL-resolution grid: the caller sends it to scratch,
      // and the 2x2 sum pass behind it owns the ReLU mask and the accumulation
      a.wt = filters(mfma_prepared_rot(d));
      a.PT = d->kh - 1 - a.PT; a.PL = d->kw - 1 - a.PL;
      if (up) a.accumulate = 0;
    }
  }
  return RCGAN_OK;
}

int rcgan_conv2d_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, void* y) {
  return rcgan_conv2d_fwd_residual(ctx, d, x, prepared, bias, nullptr, y);
}

// ---- batch-norm statistics out of the producing convolution's epilogue (conv_mfma8.hip) -------------------------------------
int rcgan_conv_stats_ok(const rcgan_conv_desc* d) {
  if (!d || !mfma_eligible(d) || d->stride != 1 || d->cout != 256) return 0;
  if (d->flags & (RCGAN_CONV_OUT_MEANPOOL2 | RCGAN_CONV_ACCUMULATE | RCGAN_CONV_IN_RELU | RCGAN_CONV_FORCE_DIRECT)) return 0;
  if (((long)d->n * d->h * d->w) % 256 != 0) return 0;
  if ((d->flags & RCGAN_CONV_RESID_UPSAMPLE2X) && !rcgan_conv_resid_up_ok(d)) return 0;
  // (asked with stats == nullptr although the launch sets it: the routing reads !a.stats only to choose between the halo-patch and the
  // tile-per-tap 256 x 256 kernel, and mfma_conv_is_p8 says yes to both)
  MfmaConvArgs a;
  if (mfma_conv_pose(nullptr, d, CONV_FWD, nullptr, nullptr, nullptr, false, nullptr, &a)) return 0;
  // (an upsample-3x3 layer must take its sub-pixel form or not be upsampled at all: the finisher knows these two tile orders)
  if (a.up && !(mfma_phase_filters(d) && mfma_conv8_phase_form(a))) return 0;
  return mfma_conv_is_p8(a) ? 1 : 0;
}

size_t rcgan_conv_stats_bytes(const rcgan_conv_desc* d) {
  return d ? (size_t)((long)d->n * d->h * d->w / 256) * d->cout * 2 * sizeof(float) : 0;
}

int rcgan_conv2d_fwd_stats(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias,
                           const void* residual, void* y, float* tile_sums) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, tile_sums != nullptr, "null tile_sums");
  RC_REQUIRE(ctx, rcgan_conv_stats_ok(d), "this convolution does not produce tile statistics (rcgan_conv_stats_ok)");
  MfmaConvArgs a;
  rc = mfma_conv_pose(ctx, d, CONV_FWD, x, prepared, bias, residual != nullptr, y, &a);
  if (rc) return rc;
  a.resid = (const bf16_t*)residual;
  a.stats = tile_sums;
  return mfma_conv_launch(ctx, a);
}

int rcgan_bn_stats_from_tiles(rcgan_ctx* ctx, const rcgan_conv_desc* d, int nseg, float eps, const float* tile_sums, float* mean, float* rstd) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, rcgan_conv_stats_ok(d) && tile_sums && mean && rstd, "bad arguments");
  RC_REQUIRE(ctx, nseg >= 1 && d->n % nseg == 0, "%d samples in %d segments", d->n, nseg);
  const long px = (long)d->h * d->w;                  // output pixels per sample
  const double count = (double)(d->n / nseg) * (double)px;
  if (d->flags & RCGAN_CONV_IN_UPSAMPLE2X) {
    // sub-pixel form: tile index = (phase, sample, low-resolution pixels / 256)
    const long tps = px / 4 / 256;                    // tiles per sample and phase
    RC_REQUIRE(ctx, tps >= 1 && (px / 4) % 256 == 0, "sub-pixel tiles must hold whole 256-pixel runs of one sample");
    return bn_tile_stats_finish_launch(ctx, tile_sums, d->cout, nseg, (int)((d->n / nseg) * tps), 4, (long)d->n * tps, count, eps, mean, rstd);
  }
  RC_REQUIRE(ctx, px % 256 == 0 || 256 % px == 0, "tiles must not straddle segments");
  RC_REQUIRE(ctx, ((long)(d->n / nseg) * px) % 256 == 0, "a segment must be whole tiles");
  return bn_tile_stats_finish_launch(ctx, tile_sums, d->cout, nseg, (int)((long)(d->n / nseg) * px / 256), 1, 0, count, eps, mean, rstd);
}

// the convolutions that can apply the batch norm in front of them to their staged input: the small-output image-end layers (G.Output)
// and (round 5) whatever the routing hands to a halo-patch kernel -- plain 3x3 / upsample-3x3 layers on 16- / 32-wide (low-resolution)
// images with enough tiles to fill the chip (G.Block.2.Conv2, G.Block.3.Conv1 / Conv2 at the bench batches)
static int mfma_bn_in_route(const rcgan_conv_desc* d) {
  if (!d || d->dtype != RCGAN_H16 || !mfma_eligible(d) || (d->flags & (RCGAN_CONV_OUT_MEANPOOL2 | RCGAN_CONV_IN_RELU | RCGAN_CONV_ACCUMULATE | RCGAN_CONV_FORCE_DIRECT)))
    return 0;
  static const int on = [] { const char* e = getenv("RCGAN_BN_INTO_PATCH"); return e ? atoi(e) : 1; }();
  if (!on) return 0;
  MfmaConvArgs a;
  if (mfma_conv_pose(nullptr, d, CONV_FWD, nullptr, nullptr, nullptr, false, nullptr, &a)) return 0;
  return mfma_conv_bn_route(a);
}

int rcgan_conv_bn_in_ok(const rcgan_conv_desc* d) {
  return (d && d->dtype == RCGAN_H16 && (img_fwd_bn_ok(d) || mfma_bn_in_route(d))) ? 1 : 0;
}

int rcgan_conv2d_fwd_bn(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, void* y,
                        int segments, const int32_t* labels, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        int act) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, x && prepared && y, "null argument");
  return rcgan_conv2d_fwd_bn_residual(ctx, d, x, prepared, bias, nullptr, y, segments, labels, gamma, beta, mean, rstd, act);
}

int rcgan_conv2d_fwd_bn_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias, const void* residual,
                                 void* y, int segments, const int32_t* labels, const float* gamma, const float* beta, const float* mean,
                                 const float* rstd, int act) {
  if (!ctx) return RCGAN_EINVALID_ARG;
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, x && prepared && y && mean && rstd && gamma && beta, "null argument");
  RC_REQUIRE(ctx, segments >= 1 && d->n % segments == 0, "segments must divide the batch");
  if (!rcgan_conv_bn_in_ok(d)) RC_FAIL(ctx, RCGAN_EUNSUPPORTED_SHAPE, "no kernel applies a batch norm to this convolution's staged input (rcgan_conv_bn_in_ok)");
  if (residual == nullptr && img_fwd_bn_ok(d)) return img_fwd_bn(ctx, d, x, prepared, bias, y, mean, rstd, gamma, beta, labels, segments, act);
  RC_REQUIRE(ctx, mfma_bn_in_route(d), "residual form needs a halo-patch kernel");
  MfmaConvArgs a;
  rc = mfma_conv_pose(ctx, d, CONV_FWD, x, prepared, bias, residual != nullptr, y, &a);
  if (rc) return rc;
  rc = ensure_selftest(ctx);
  if (rc) return rc;
  a.resid = (const bf16_t*)residual;
  a.bn_mean = mean; a.bn_rstd = rstd; a.bn_gamma = gamma; a.bn_beta = beta; a.bn_labels = labels;
  a.bn_seg_samples = d->n / segments; a.bn_act = act;
  return mfma_conv_launch(ctx, a);
}

int rcgan_conv2d_fwd_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* prepared, const float* bias,
                              const void* residual, void* y) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  if (residual != nullptr && !mfma_eligible(d)) {      // other kernels: plain forward, then y += residual
    RC_REQUIRE(ctx, !(d->flags & RCGAN_CONV_RESID_UPSAMPLE2X), "half-resolution residual not available for this convolution (rcgan_conv_resid_up_ok)");
    RC_REQUIRE(ctx, residual != y, "residual must not alias the output");
    rc = rcgan_conv2d_fwd_residual(ctx, d, x, prepared, bias, nullptr, y);
    if (rc) return rc;
    int oh, ow, p;
    same_pad(d->h, d->kh, d->stride, &oh, &p);
    same_pad(d->w, d->kw, d->stride, &ow, &p);
    return rcgan_axpby(ctx, (size_t)d->n * oh * ow * d->cout, d->dtype, 1.f, residual, 1.f, y);
  }
  if ((d->flags & RCGAN_CONV_OUT_MEANPOOL2) || mfma_eligible(d)) {
    MfmaConvArgs a;
    rc = mfma_conv_pose(ctx, d, CONV_FWD, x, prepared, bias, residual != nullptr, y, &a);
    if (rc) return rc;
    a.resid = (const bf16_t*)residual;
    return mfma_conv_launch(ctx, a);
  }
  if (img_side(d)) return img_fwd(ctx, d, x, prepared, bias, y);
  if (int kind = small_fwd_kind(d)) {
    RC_DISPATCH_DTYPE(ctx, d->dtype, return small_fwd<T>(ctx, d, kind, (const T*)x, (const float*)prepared, bias, (T*)y));
  }
  RC_DISPATCH_DTYPE(ctx, d->dtype, return direct_fwd<T>(ctx, d, (const T*)x, (const float*)prepared, nullptr, bias, (T*)y));
  return RCGAN_OK;
}

int rcgan_conv2d_bwd_data(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* prepared, const void* x, void* dx,
                          void* ws, size_t ws_bytes) {
  return rcgan_conv2d_bwd_data_residual(ctx, d, dy, prepared, x, nullptr, dx, ws, ws_bytes);
}

int rcgan_conv2d_bwd_data_residual(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const void* prepared, const void* x,
                                   const void* residual, void* dx, void* ws, size_t ws_bytes) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  if (residual != nullptr) {
    RC_REQUIRE(ctx, residual != dx && !(d->flags & RCGAN_CONV_ACCUMULATE), "residual form is out of place and not accumulating");
    if (!mfma_eligible(d) || (d->flags & RCGAN_CONV_IN_UPSAMPLE2X)) {      // other kernels: plain data gradient, then dx += residual
      rc = rcgan_conv2d_bwd_data_residual(ctx, d, dy, prepared, x, nullptr, dx, ws, ws_bytes);
      if (rc) return rc;
      return rcgan_axpby(ctx, (size_t)d->n * d->h * d->w * d->cin, d->dtype, 1.f, residual, 1.f, dx);
    }
  }
  const bool up = d->flags & RCGAN_CONV_IN_UPSAMPLE2X;
  const bool relu = d->flags & RCGAN_CONV_IN_RELU;
  const int acc = (d->flags & RCGAN_CONV_ACCUMULATE) ? 1 : 0;
  RC_REQUIRE(ctx, !relu || x != nullptr, "IN_RELU needs x for the mask");
  void* target = dx;
  if (up) {
    size_t need = (size_t)d->n * d->h * d->w * d->cin * dtype_size(d->dtype);
    if (ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
    target = ws;
  }
  const void* mask = (relu && !up) ? x : nullptr;
  const int acc_now = up ? 0 : acc;
  if ((d->flags & RCGAN_CONV_OUT_MEANPOOL2) || mfma_eligible(d)) {
    MfmaConvArgs a;
    rc = mfma_conv_pose(ctx, d, CONV_DGRAD, dy, prepared, nullptr, residual != nullptr, dx, &a);
    if (rc) return rc;
    // an upsampled layer not taken in gather form: full-resolution dx into the scratch, mask and accumulation in the sum pass below
    const bool scratch = up && a.phase == MFMA_FORM_PLAIN;
    if (scratch) a.out = (bf16_t*)target;
    a.mask = (relu && !scratch) ? (const bf16_t*)x : nullptr;
    a.resid = (const bf16_t*)residual;
    rc = mfma_conv_launch(ctx, a);
    if (rc || !scratch) return rc;
  } else if (mask == nullptr && !up && img_side(d)) {
    rc = img_dgrad(ctx, d, dy, prepared, target, acc_now);
    if (rc) return rc;
  } else if (int kind = (mask == nullptr && !up) ? small_dgrad_kind(d) : 0) {
    RC_DISPATCH_DTYPE(ctx, d->dtype, rc = small_dgrad<T>(ctx, d, kind, (const T*)dy, (const float*)prepared, (T*)target, acc_now));
    if (rc) return rc;
  } else {
    RC_DISPATCH_DTYPE(ctx, d->dtype, rc = direct_dgrad<T>(ctx, d, (const T*)dy, (const float*)prepared, nullptr, nullptr, (const T*)mask, (T*)target, acc_now));
    if (rc) return rc;
  }
  if (up) {
    RC_DISPATCH_DTYPE(ctx, d->dtype, rc = sumpool2_masked_launch<T>(ctx, d->n, d->h, d->w, d->cin, (const T*)ws, relu ? (const T*)x : (const T*)nullptr, (T*)dx, acc));
    if (rc) return rc;
  }
  return RCGAN_OK;
}

// transposed conv: d describes the forward conv whose data-gradient it is (see header)
int rcgan_deconv2d_fwd(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const float* w, const float* bias, void* y) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_DISPATCH_DTYPE(ctx, d->dtype, return direct_dgrad<T>(ctx, d, (const T*)x, w, nullptr, bias, (const T*)nullptr, (T*)y, 0));
  return RCGAN_OK;
}

int rcgan_deconv2d_bwd_data(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const float* w, void* dx) {
  return rcgan_deconv2d_bwd_data_cols(ctx, d, dy, w, dx, 0);
}

int rcgan_deconv2d_bwd_data_cols(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* dy, const float* w, void* dx, int n_cols) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, n_cols >= 0 && n_cols <= d->cout, "n_cols %d of %d input channels", n_cols, d->cout);
  RC_DISPATCH_DTYPE(ctx, d->dtype, return direct_fwd<T>(ctx, d, (const T*)dy, w, nullptr, nullptr, (T*)dx, n_cols));
  return RCGAN_OK;
}

int rcgan_deconv2d_bwd_weight(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias,
                              int accumulate, void* ws, size_t ws_bytes) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  // forward-conv input = deconv output gradient dy; forward-conv output gradient = deconv input x
  RC_DISPATCH_DTYPE(ctx, d->dtype, rc = direct_wgrad<T>(ctx, d, (const T*)dy, (const T*)x, dw, nullptr, accumulate, ws, ws_bytes));
  if (rc) return rc;
  if (dbias) {
    int oh, ow, p;
    same_pad(d->h, d->kh, d->stride, &oh, &p);
    same_pad(d->w, d->kw, d->stride, &ow, &p);
    (void)oh; (void)ow;
    long rows = (long)d->n * d->h * d->w;
    // partial column sums go to the tail of the workspace (the filter-gradient slabs sit at its head and are consumed)
    size_t need = colsum_tail_bytes(rows, d->cin);
    float* part = (ws != nullptr && ws_bytes >= direct_wgrad_ws_bytes(d) + need) ? (float*)((char*)ws + (ws_bytes - need) / 256 * 256) : nullptr;
    RC_DISPATCH_DTYPE(ctx, d->dtype, rc = colsum_launch<T>(ctx, (const T*)dy, rows, d->cin, dbias, accumulate, part));
    if (rc) return rc;
  }
  return RCGAN_OK;
}

size_t rcgan_deconv2d_bwd_weight_concat_bytes(const rcgan_conv_desc* d, int n_cols) {
  if (!d || n_cols <= 0 || n_cols >= d->cout) return 0;
  const long rows = (long)d->n * d->h * d->w;
  return direct_wgrad_cols_ws_bytes(d, n_cols) + colsum_tail_bytes(rows, d->cin) + 256;
}

int rcgan_deconv2d_bwd_weight_concat(rcgan_ctx* ctx, const rcgan_conv_desc* d, const void* x, const void* dy, int n_cols, const float* yb,
                                     float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes) {
  int rc = check_desc(ctx, d);
  if (rc) return rc;
  RC_REQUIRE(ctx, n_cols > 0 && n_cols < d->cout && yb != nullptr, "%d real columns of %d, yb %p", n_cols, d->cout, (const void*)yb);
  const size_t need = rcgan_deconv2d_bwd_weight_concat_bytes(d, n_cols);
  if (ws == nullptr || ws_bytes < need) RC_FAIL(ctx, RCGAN_EWORKSPACE_TOO_SMALL, "need %zu have %zu", need, ws_bytes);
  // forward-conv input = deconv output gradient dy; forward-conv output gradient = deconv input x = [t ; yb]
  RC_DISPATCH_DTYPE(ctx, d->dtype, rc = direct_wgrad_cols<T>(ctx, d, (const T*)dy, (const T*)x, n_cols, yb, dw, accumulate, ws, ws_bytes));
  if (rc) return rc;
  if (dbias) {
    const long rows = (long)d->n * d->h * d->w;
    const size_t tail = colsum_tail_bytes(rows, d->cin);
    float* part = (float*)((char*)ws + (ws_bytes - tail) / 256 * 256);
    RC_DISPATCH_DTYPE(ctx, d->dtype, rc = colsum_launch<T>(ctx, (const T*)dy, rows, d->cin, dbias, accumulate, part));
    if (rc) return rc;
  }
  return RCGAN_OK;
}

// ------------------------------------------------------------------------------------------------
// dense layers: plain row-major GEMMs on the shared fp32 GEMM core (conv_direct.hip)
// ------------------------------------------------------------------------------------------------
static int check_lin(rcgan_ctx* ctx, int m, int k, int n, int dtype) {
  RC_REQUIRE(ctx, m > 0 && k > 0 && n > 0, "bad linear shape [%d,%d]x[%d,%d]", m, k, k, n);
  RC_REQUIRE(ctx, dtype == RCGAN_F32 || dtype == RCGAN_H16, "bad dtype %d", dtype);
  return RCGAN_OK;
}

size_t rcgan_linear_workspace_bytes(int m, int k, int n) { return linear_wgrad_ws_bytes(m, k, n); }

int rcgan_linear_fwd(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* x, const float* w, const float* sigma,
                     const float* bias, void* y) {
  int rc = check_lin(ctx, m, k, n, dtype);
  if (rc) return rc;
  RC_DISPATCH_DTYPE(ctx, dtype, return linear_fwd<T>(ctx, m, k, n, (const T*)x, w, sigma, bias, (T*)y));
  return RCGAN_OK;
}

int rcgan_linear_bwd_data(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* dy, const float* w, const float* sigma,
                          void* dx, int accumulate) {
  int rc = check_lin(ctx, m, k, n, dtype);
  if (rc) return rc;
  RC_DISPATCH_DTYPE(ctx, dtype, return linear_dgrad<T>(ctx, m, k, n, (const T*)dy, w, sigma, (T*)dx, accumulate));
  return RCGAN_OK;
}

int rcgan_linear_bwd_weight(rcgan_ctx* ctx, int m, int k, int n, int dtype, const void* x, const void* dy, float* dw, float* dbias,
                            int accumulate, void* ws, size_t ws_bytes) {
  int rc = check_lin(ctx, m, k, n, dtype);
  if (rc) return rc;
  RC_DISPATCH_DTYPE(ctx, dtype, return linear_wgrad<T>(ctx, m, k, n, (const T*)x, (const T*)dy, dw, dbias, accumulate, ws, ws_bytes));
  return RCGAN_OK;
}

// ------------------------------------------------------------------------------------------------
// optimiser
// ------------------------------------------------------------------------------------------------
int rcgan_adam_tf(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v, const float* hyper, float beta1,
                  float beta2, float eps, float clip, float grad_scale) {
  if (count == 0) return RCGAN_OK;
  RC_REQUIRE(ctx, hyper != nullptr, "null hyper (rcgan_adam_tf_host takes {lr, t} by value)");
  adam_launch(ctx, count, w, g, m, v, hyper, 0.f, 0.f, beta1, beta2, eps, clip, grad_scale);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_adam_tf_host(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v, float lr, float t, float beta1,
                       float beta2, float eps, float clip, float grad_scale) {
  if (count == 0) return RCGAN_OK;
  adam_launch(ctx, count, w, g, m, v, nullptr, lr, t, beta1, beta2, eps, clip, grad_scale);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_set2_f32(rcgan_ctx* ctx, float* p, float a, float b) {
  RC_REQUIRE(ctx, p != nullptr, "null pointer");
  hipLaunchKernelGGL(set2_kernel, dim3(1), dim3(1), 0, ctx->stream, p, a, b);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_set_grad_scale(rcgan_ctx* ctx, float host_scale, const float* dev_scale) {
  RC_REQUIRE(ctx, host_scale > 0.f, "grad scale %g", (double)host_scale);
  ctx->gscale_host = host_scale;
  ctx->gscale_dev = dev_scale;
  return RCGAN_OK;
}

int rcgan_grad_finite_check(rcgan_ctx* ctx, size_t count, const float* g, float* ls_state) {
  RC_REQUIRE(ctx, g != nullptr && ls_state != nullptr && ((size_t)g & 15) == 0, "null / misaligned argument");
  if (count == 0) return RCGAN_OK;
  size_t blocks = (count / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(grad_finite_check_kernel, dim3((int)blocks), dim3(256), 0, ctx->stream, count, g, ls_state);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_adam_tf_dyn(rcgan_ctx* ctx, size_t count, float* w, const float* g, float* m, float* v, float lr, const float* t_dev, float beta1,
                      float beta2, float eps, float clip, float grad_scale, const float* ls_state) {
  RC_REQUIRE(ctx, t_dev != nullptr && ls_state != nullptr, "null t_dev / ls_state");
  if (count == 0) return RCGAN_OK;
  adam_launch(ctx, count, w, g, m, v, nullptr, lr, 0.f, beta1, beta2, eps, clip, grad_scale, AdamDyn{ls_state, t_dev});
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

int rcgan_loss_scale_update(rcgan_ctx* ctx, float* ls_state, float* t_dev0, float* t_dev1, float growth_interval, float min_scale,
                            float max_scale) {
  RC_REQUIRE(ctx, ls_state != nullptr && growth_interval >= 1.f && min_scale > 0.f && max_scale >= min_scale, "bad loss-scale arguments");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, ctx->stream, ls_state, t_dev0, t_dev1, growth_interval, min_scale, max_scale);
  RC_LAUNCH_CHECK(ctx);
  return RCGAN_OK;
}

}  // extern "C"
