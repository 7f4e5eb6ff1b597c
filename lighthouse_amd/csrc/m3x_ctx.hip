// The library's context, buffer and timing C-ABI, and the host helpers every
// other unit links against (m3x_ctx.hh): context create/destroy, device
// buffers and copies, per-kernel event timing, growable scratch. The one
// kernel here fills the context's zero-hash ladder at create.
#include "merkle_node.hh"
#include "m3x_ctx.hh"
#include "../../include/m3x_consensus.h"

using namespace m3x;

// single-thread: Z[0]=0^32, Z[i]=H(Z[i-1]||Z[i-1]) (merkle_proof ZERO_NODES)
__global__ void k_zero_ladder(uint8_t *zeros /*65*32*/) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t z[8];
#pragma unroll
  for (int i = 0; i < 8; i++) z[i] = 0;
  store_node(zeros, z);
  for (int lvl = 1; lvl <= 64; lvl++) {
    uint32_t o[8];
    sha256_node(z, z, o);
#pragma unroll
    for (int i = 0; i < 8; i++) z[i] = o[i];
    store_node(zeros + 32 * lvl, z);
  }
}

namespace m3x {
void time_begin_s(m3x_ctx *ctx, int k, hipStream_t st) {
  if (!ctx->timing) return;
  if (!ctx->ev_a[k]) {
    (void)hipEventCreate(&ctx->ev_a[k]);
    (void)hipEventCreate(&ctx->ev_b[k]);
  }
  (void)hipEventRecord(ctx->ev_a[k], st);
}

void time_end_s(m3x_ctx *ctx, int k, hipStream_t st) {
  if (!ctx->timing) return;
  (void)hipEventRecord(ctx->ev_b[k], st);
  (void)hipEventSynchronize(ctx->ev_b[k]);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev_a[k], ctx->ev_b[k]);
  ctx->kernel_ms[k] += ms;
  ctx->kernel_launches[k]++;
}

void time_begin(m3x_ctx *ctx, int k) { time_begin_s(ctx, k, ctx->stream); }
void time_end(m3x_ctx *ctx, int k) { time_end_s(ctx, k, ctx->stream); }

int ensure_scratch(m3x_ctx *ctx, uint8_t **buf, uint64_t *cur,
                   uint64_t bytes) {
  if (*cur >= bytes) return M3X_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *cur = 0;
  if (hipMalloc(buf, bytes) != hipSuccess) return M3X_ERR_NOMEM;
  *cur = bytes;
  return M3X_OK;
}
} // namespace m3x

// everything m3x_ctx_create does after `new`; on failure the caller hands
// the partly built context to m3x_ctx_destroy
static int32_t ctx_init(m3x_ctx *ctx) {
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  M3X_HIP_CHECK(hipStreamCreate(&ctx->stream));
  M3X_HIP_CHECK(hipStreamCreate(&ctx->stream2));
  M3X_HIP_CHECK(hipStreamCreate(&ctx->stream3));
  M3X_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_s2, hipEventDisableTiming));
  for (hipEvent_t &ev : ctx->ev_pipe)
    M3X_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (hipMalloc(&ctx->zeros_dev, 65 * 32) != hipSuccess ||
      hipMalloc(&ctx->small_pool, m3x_ctx::SMALL_POOL_IN + 64) != hipSuccess)
    return M3X_ERR_NOMEM;
  hipLaunchKernelGGL(k_zero_ladder, dim3(1), dim3(64), 0, ctx->stream,
                     ctx->zeros_dev);
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return M3X_OK;
}

extern "C" {

int32_t m3x_abi_version(void) { return 1; }

int32_t m3x_ctx_create(m3x_ctx **out, int32_t device) {
  auto *ctx = new m3x_ctx();
  ctx->device = device;
  int32_t rc = ctx_init(ctx);
  if (rc != M3X_OK) {
    m3x_ctx_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return M3X_OK;
}

void m3x_ctx_destroy(m3x_ctx *ctx) {
  if (!ctx) return;
  if (ctx->zeros_dev) (void)hipFree(ctx->zeros_dev);
  if (ctx->small_pool) (void)hipFree(ctx->small_pool);
  if (ctx->scratch_a) (void)hipFree(ctx->scratch_a);
  if (ctx->scratch_b) (void)hipFree(ctx->scratch_b);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
  if (ctx->ev_s2) (void)hipEventDestroy(ctx->ev_s2);
  for (hipEvent_t ev : ctx->ev_pipe)
    if (ev) (void)hipEventDestroy(ev);
  delete ctx;
}

int32_t m3x_dev_alloc(m3x_ctx *ctx, uint64_t bytes, void **dev_ptr) {
  if (!ctx || !dev_ptr) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  M3X_HIP_CHECK(hipMalloc(dev_ptr, bytes));
  return M3X_OK;
}

int32_t m3x_dev_free(m3x_ctx *ctx, void *dev_ptr) {
  if (!ctx) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipFree(dev_ptr));
  return M3X_OK;
}

int32_t m3x_h2d(m3x_ctx *ctx, void *dst_dev, const void *src_host,
                uint64_t bytes) {
  if (!ctx) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  M3X_HIP_CHECK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice,
                               ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return M3X_OK;
}

int32_t m3x_d2h(m3x_ctx *ctx, void *dst_host, const void *src_dev,
                uint64_t bytes) {
  if (!ctx) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  M3X_HIP_CHECK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost,
                               ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return M3X_OK;
}

int32_t m3x_timing_enable(m3x_ctx *ctx, int32_t on) {
  if (!ctx) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  ctx->timing = on != 0;
  for (int i = 0; i < M3X_K_COUNT; i++) {
    ctx->kernel_ms[i] = 0;
    ctx->kernel_launches[i] = 0;
  }
  return M3X_OK;
}

int32_t m3x_kernel_ms(m3x_ctx *ctx, int32_t kernel_id, double *ms,
                      uint64_t *launches) {
  if (!ctx || kernel_id < 0 || kernel_id >= M3X_K_COUNT ||
      kernel_id == M3X_K_RESERVED_25)
    return M3X_ERR_ARG;
  *ms = ctx->kernel_ms[kernel_id];
  *launches = ctx->kernel_launches[kernel_id];
  return M3X_OK;
}

} // extern "C"
