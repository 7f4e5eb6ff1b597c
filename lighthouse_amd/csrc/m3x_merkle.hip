// MI355X-native SSZ merkleization (hot path #2) and the incremental
// registry cache. The context, buffer and timing C-ABI is m3x_ctx.hip.
//
// Replaces BeaconState::update_tree_hash_cache's SHA256 merkleize
// (consensus/types/src/beacon_state.rs:2031-2046; math restated from
// merkle_proof/src/lib.rs:9-14,68-100, mix_in_length from
// deposit_data_tree.rs:26-38, Validator layout from validator.rs:25-35,
// 2^40 registry limit from eth_spec.rs:404). Designed CDNA4-first: one
// validator / one two-to-one node per lane (wave64), the padding-block
// compression constant-folded, multi-level LDS reduction per workgroup,
// grids ≫256 blocks to fill 8 XCDs. Integer VALU workload — no MFMA, HBM
// traffic ≈96B per node (see DESIGN.md roofline).
#include "merkle_node.hh"
#include "m3x_ctx.hh"
#include "../../include/m3x_consensus.h"
#include <memory>

using namespace m3x;

// ------------------------------------------------------------------ kernels

__device__ __forceinline__ uint32_t be_load_u8x4(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
         ((uint32_t)p[2] << 8) | p[3];
}

// Z[level] of the context's zero ladder
__device__ __forceinline__ void load_zero(const uint8_t *zeros, uint32_t level,
                                          uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = be_load_u8x4(zeros + 32 * level + 4 * i);
}

// dst32 = H(src64[0:32] || src64[32:64]), nodes in device memory
__device__ __forceinline__ void hash_pair(const uint8_t *src64,
                                          uint8_t *dst32) {
  uint32_t l[8], r[8], o[8];
  load_node(src64, l);
  load_node(src64 + 32, r);
  sha256_node(l, r, o);
  store_node(dst32, o);
}

// Validator hash_tree_root of one 121B SSZ record (any alignment, LDS or
// global): 8 two-to-one hashes, pubkey root + 7 field-tree nodes. Stays
// force-inlined so the address space of `rec` reaches the byte loads.
__device__ __forceinline__ void validator_leaf_root(const uint8_t *rec,
                                                    uint32_t root[8]) {
  // field chunks (big-endian words for the hasher); layout validator.rs:25-35
  uint32_t c[8][8];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 8; j++) c[i][j] = 0;
  // c0 = H(pk[0:32] || pk[32:48] + 16 zero bytes)
  {
    uint32_t l[8], r[8];
#pragma unroll
    for (int i = 0; i < 8; i++) l[i] = be_load_u8x4(rec + 4 * i);
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = be_load_u8x4(rec + 32 + 4 * i);
#pragma unroll
    for (int i = 4; i < 8; i++) r[i] = 0;
    sha256_node(l, r, c[0]);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) c[1][i] = be_load_u8x4(rec + 48 + 4 * i); // wc
  c[2][0] = be_load_u8x4(rec + 80); // effective_balance LE bytes as-is
  c[2][1] = be_load_u8x4(rec + 84);
  c[3][0] = (uint32_t)rec[88] << 24; // slashed bool in byte 0 of the chunk
  c[4][0] = be_load_u8x4(rec + 89);
  c[4][1] = be_load_u8x4(rec + 93);
  c[5][0] = be_load_u8x4(rec + 97);
  c[5][1] = be_load_u8x4(rec + 101);
  c[6][0] = be_load_u8x4(rec + 105);
  c[6][1] = be_load_u8x4(rec + 109);
  c[7][0] = be_load_u8x4(rec + 113);
  c[7][1] = be_load_u8x4(rec + 117);
  // 8-leaf tree: 4 + 2 + 1 hashes
  uint32_t h01[8], h23[8], h45[8], h67[8], ha[8], hb[8];
  sha256_node(c[0], c[1], h01);
  sha256_node(c[2], c[3], h23);
  sha256_node(c[4], c[5], h45);
  sha256_node(c[6], c[7], h67);
  sha256_node(h01, h23, ha);
  sha256_node(h45, h67, hb);
  sha256_node(ha, hb, root);
}

// Validator hash_tree_root leaves: one lane = one validator (121B SSZ ->
// 32B root). The block cooperatively stages its 256*121 contiguous bytes
// through LDS with coalesced u32 loads, then each lane hashes its record.
__global__ __launch_bounds__(256) void k_validator_leaves(
    const uint8_t *__restrict__ ssz, uint64_t n, uint8_t *__restrict__ out) {
  __shared__ uint8_t lds[256 * 121 + 4];
  uint64_t base_rec = (uint64_t)blockIdx.x * 256;
  const uint32_t block_bytes = 256 * 121; // 30976, divisible by 4
  uint64_t gbase = base_rec * 121;
  uint64_t total = n * 121;
  // coalesced staging (u32 granularity; source is 4-byte aligned per block)
  for (uint32_t i = threadIdx.x; i < block_bytes / 4; i += 256) {
    uint64_t goff = gbase + 4ull * i;
    uint32_t v = 0;
    if (goff + 4 <= total) {
      v = *reinterpret_cast<const uint32_t *>(ssz + goff);
    } else if (goff < total) {
      // ragged tail of the whole array
      uint32_t b0 = ssz[goff];
      uint32_t b1 = (goff + 1 < total) ? ssz[goff + 1] : 0;
      uint32_t b2 = (goff + 2 < total) ? ssz[goff + 2] : 0;
      v = b0 | (b1 << 8) | (b2 << 16);
    }
    *reinterpret_cast<uint32_t *>(lds + 4 * i) = v;
  }
  __syncthreads();
  uint64_t rec = base_rec + threadIdx.x;
  if (rec >= n) return;
  uint32_t root[8];
  validator_leaf_root(lds + 121 * threadIdx.x, root);
  store_node(out + 32 * rec, root);
}

// Multi-level reduction: each block folds 2^levels consecutive input nodes
// (levels <= 9) into one output node through LDS double buffers. Missing
// trailing nodes are the zero ladder Z[base_level] (padding with ladder
// values is exactly the right-sparse semantics of merkle_proof::create).
__global__ __launch_bounds__(256) void k_reduce(
    const uint8_t *__restrict__ in, uint64_t n_in, uint8_t *__restrict__ out,
    uint32_t levels, uint32_t base_level, const uint8_t *__restrict__ zeros) {
  __shared__ uint32_t A[512][8];
  __shared__ uint32_t B[256][8];
  const uint32_t span = 1u << levels; // <= 512
  uint64_t base = (uint64_t)blockIdx.x * span;
  uint32_t zw[8];
  load_zero(zeros, base_level, zw);
  // load span nodes (each thread loads up to 2)
  for (uint32_t s = threadIdx.x; s < span; s += 256) {
    uint64_t idx = base + s;
    if (idx < n_in) {
      load_node(in + 32 * idx, A[s]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) A[s][i] = zw[i];
    }
  }
  __syncthreads();
  uint32_t cnt = span;
  for (uint32_t l = 0; l < levels; l++) {
    uint32_t half = cnt >> 1;
    if (l % 2 == 0) { // A -> B
      for (uint32_t t = threadIdx.x; t < half; t += 256)
        sha256_node(A[2 * t], A[2 * t + 1], B[t]);
    } else { // B -> A
      for (uint32_t t = threadIdx.x; t < half; t += 256)
        sha256_node(B[2 * t], B[2 * t + 1], A[t]);
    }
    cnt = half;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    store_node(out + 32 * blockIdx.x, (levels % 2 == 1) ? B[0] : A[0]);
}

// single-thread finalize: carry node from `from_level` to `to_depth` against
// the zero ladder (node is always the LEFT child — right-sparse tree), then
// optionally mix_in_length.
__global__ void k_finalize(const uint8_t *__restrict__ node_in,
                           uint32_t from_level, uint32_t to_depth,
                           int64_t mix_len, const uint8_t *__restrict__ zeros,
                           uint8_t *__restrict__ out32) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t node[8];
  load_node(node_in, node);
  for (uint32_t l = from_level; l < to_depth; l++) {
    uint32_t z[8], o[8];
    load_zero(zeros, l, z);
    sha256_node(node, z, o);
#pragma unroll
    for (int i = 0; i < 8; i++) node[i] = o[i];
  }
  if (mix_len >= 0) {
    // length chunk: LE64(len) || zeros  (deposit_data_tree.rs:26-38)
    uint64_t len = (uint64_t)mix_len;
    uint32_t lc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    lc[0] = __builtin_bswap32((uint32_t)(len & 0xffffffffu));
    lc[1] = __builtin_bswap32((uint32_t)(len >> 32));
    uint32_t o[8];
    sha256_node(node, lc, o);
#pragma unroll
    for (int i = 0; i < 8; i++) node[i] = o[i];
  }
  store_node(out32, node);
}

// Batched small-container merkleize: one thread folds one element's chunk
// group (<=32 chunks, depth = ceil_log2(count)) — the BeaconState's many
// tiny containers (Fork, headers, Eth1Data votes, checkpoints,
// HistoricalSummary, payload header) in ONE launch.
__global__ void k_merkleize_batch(const uint8_t *__restrict__ chunks,
                                  const uint32_t *__restrict__ offs,
                                  uint64_t n, const uint8_t *__restrict__ zeros,
                                  uint8_t *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c0 = offs[i], c1 = offs[i + 1];
  uint32_t cnt = c1 - c0;
  uint32_t node[32][8];
  for (uint32_t j = 0; j < cnt && j < 32; j++)
    load_node(chunks + 32ull * (c0 + j), node[j]);
  if (cnt == 0) // merkleize([], 0) is the zero chunk
    for (int q = 0; q < 8; q++) node[0][q] = 0;
  uint32_t depth = 0;
  while ((1u << depth) < cnt) depth++;
  uint32_t m = cnt, level = 0;
  while (level < depth) {
    uint32_t nx = (m + 1) / 2;
    for (uint32_t q = 0; q < nx; q++) {
      uint32_t zw[8];
      const uint32_t *r;
      if (2 * q + 1 < m) {
        r = node[2 * q + 1];
      } else {
        load_zero(zeros, level, zw);
        r = zw;
      }
      uint32_t o[8];
      sha256_node(node[2 * q], r, o);
      for (int b = 0; b < 8; b++) node[q][b] = o[b];
    }
    m = nx;
    level++;
  }
  store_node(out + 32 * i, node[0]);
}

// ---------------------------------------------------------------- host side

// copy a 32B root back from the device and wait for the call's stream
static int32_t read_root(m3x_ctx *ctx, const uint8_t *root_dev,
                         uint8_t out_root[32]) {
  int32_t rc = M3X_OK;
  if (hipMemcpyAsync(out_root, root_dev, 32, hipMemcpyDeviceToHost,
                     ctx->stream) != hipSuccess)
    rc = M3X_ERR_HIP;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = M3X_ERR_HIP;
  return rc;
}

// the context's root slot: [32B result][32B intermediate] (see m3x_ctx.hh)
static uint8_t *root_slot(m3x_ctx *ctx) {
  return ctx->small_pool + m3x_ctx::SMALL_POOL_IN;
}

static void launch_finalize(m3x_ctx *ctx, const uint8_t *node_dev,
                            uint32_t from_level, uint32_t to_depth,
                            int64_t mix_len, uint8_t *out_dev) {
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, ctx->stream, node_dev,
                     from_level, to_depth, mix_len, ctx->zeros_dev, out_dev);
}

static void launch_leaves(m3x_ctx *ctx, const uint8_t *ssz_dev, uint64_t n,
                          uint8_t *leaves_dev) {
  hipLaunchKernelGGL(k_validator_leaves, dim3((uint32_t)((n + 255) / 256)),
                     dim3(256), 0, ctx->stream, ssz_dev, n, leaves_dev);
}

// Reduce an array of nodes to a single subtree root at depth `depth`,
// writing the 32B root into out_dev (device).
static int32_t reduce_to_root(m3x_ctx *ctx, const uint8_t *nodes_dev,
                              uint64_t n, uint32_t depth, uint8_t *out_dev) {
  // alternate between scratch_b halves for stage outputs
  const uint8_t *cur = nodes_dev;
  uint64_t m = n;
  uint32_t level = 0;
  uint64_t need = (n + 511) / 512 * 32 + 64;
  int rc = ensure_scratch(ctx, &ctx->scratch_b, &ctx->scratch_b_bytes,
                          2 * need);
  if (rc != M3X_OK) return rc;
  uint8_t *ping = ctx->scratch_b, *pong = ctx->scratch_b + need;
  while (level < depth && m > 1) {
    uint32_t levels = depth - level < 9 ? depth - level : 9;
    uint64_t span = 1ull << levels;
    uint64_t n_out = (m + span - 1) / span;
    uint8_t *dst = (cur == ping) ? pong : ping;
    time_begin(ctx, M3X_K_REDUCE);
    hipLaunchKernelGGL(k_reduce, dim3((uint32_t)n_out), dim3(256), 0,
                       ctx->stream, cur, m, dst, levels, level,
                       ctx->zeros_dev);
    time_end(ctx, M3X_K_REDUCE);
    cur = dst;
    m = n_out;
    level += levels;
  }
  // carry to full depth (no mix here)
  launch_finalize(ctx, cur, level, depth, -1, out_dev);
  return M3X_OK;
}

// depth-`depth` subtree root of n validator records, left in out_dev
static int32_t validator_subtree_root(m3x_ctx *ctx, const uint8_t *ssz_dev,
                                      uint64_t n, uint32_t depth,
                                      uint8_t *out_dev) {
  if (n == 0) { // the ladder entry Z[depth]
    launch_finalize(ctx, ctx->zeros_dev + 32 * depth, depth, depth, -1,
                    out_dev);
    return M3X_OK;
  }
  int rc = ensure_scratch(ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, n * 32);
  if (rc != M3X_OK) return rc;
  time_begin(ctx, M3X_K_LEAVES);
  launch_leaves(ctx, ssz_dev, n, ctx->scratch_a);
  time_end(ctx, M3X_K_LEAVES);
  return reduce_to_root(ctx, ctx->scratch_a, n, depth, out_dev);
}

// device copy of n validator records, rounded up to the 4 bytes
// k_validator_leaves stages by; null when the allocation or the copy failed
static const uint8_t *upload_validators(DevTemps &tmp, const uint8_t *ssz,
                                        uint64_t n) {
  uint8_t *dev = tmp.alloc((n * 121 + 3) & ~3ull);
  if (dev && hipMemcpy(dev, ssz, n * 121, hipMemcpyHostToDevice) != hipSuccess)
    return nullptr;
  return dev;
}

extern "C" {

/* carry a 32B node from `from_level` to `to_depth` against the zero ladder,
 * then optionally mix_in_length — the multi-GPU cap-finishing primitive. */
int32_t m3x_finalize_root(m3x_ctx *ctx, const uint8_t node[32],
                          uint32_t from_level, uint32_t to_depth,
                          int64_t mix_len, uint8_t out_root[32]) {
  if (!ctx || to_depth > 64) return M3X_ERR_ARG; // the ladder ends at Z[64]
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint8_t *tmp = ctx->small_pool;
  M3X_HIP_CHECK(hipMemcpy(tmp, node, 32, hipMemcpyHostToDevice));
  launch_finalize(ctx, tmp, from_level, to_depth, mix_len, tmp + 32);
  return read_root(ctx, tmp + 32, out_root);
}

int32_t m3x_merkleize_chunks_dev(m3x_ctx *ctx, const void *chunks_dev,
                                 uint64_t n_chunks, uint32_t depth,
                                 int64_t mix_len, uint8_t out_root[32]) {
  if (!ctx || depth > 64) return M3X_ERR_ARG; // the ladder ends at Z[64]
  if (depth < 63 && n_chunks > (1ull << depth)) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint8_t *root_dev = root_slot(ctx);
  const uint8_t *node = ctx->zeros_dev + 32 * depth; // no chunks: Z[depth]
  if (n_chunks) {
    int32_t rc = reduce_to_root(ctx, (const uint8_t *)chunks_dev, n_chunks,
                                depth, root_dev + 32);
    if (rc != M3X_OK) return rc;
    node = root_dev + 32;
  }
  launch_finalize(ctx, node, depth, depth, mix_len, root_dev); // optional mix
  return read_root(ctx, root_dev, out_root);
}

int32_t m3x_merkleize_chunks(m3x_ctx *ctx, const uint8_t *chunks,
                             uint64_t n_chunks, uint32_t depth,
                             int64_t mix_len, uint8_t out_root[32]) {
  if (!ctx) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  DevTemps tmp(ctx->stream);
  const void *dev = nullptr;
  uint64_t bytes = n_chunks * 32;
  if (bytes && bytes <= m3x_ctx::SMALL_POOL_IN) {
    M3X_HIP_CHECK(
        hipMemcpy(ctx->small_pool, chunks, bytes, hipMemcpyHostToDevice));
    dev = ctx->small_pool;
  } else if (bytes) {
    dev = tmp.upload(chunks, bytes);
    if (!tmp.ok()) return M3X_ERR_HIP;
  }
  return m3x_merkleize_chunks_dev(ctx, dev, n_chunks, depth, mix_len,
                                  out_root);
}

int32_t m3x_validator_subtree_root_dev(m3x_ctx *ctx, const void *ssz_dev,
                                       uint64_t n, uint32_t depth,
                                       uint8_t out_root[32]) {
  if (!ctx || depth > 64 || (depth < 63 && n > (1ull << depth)))
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  int32_t rc = validator_subtree_root(ctx, (const uint8_t *)ssz_dev, n, depth,
                                      root_slot(ctx));
  if (rc != M3X_OK) return rc;
  return read_root(ctx, root_slot(ctx), out_root);
}

int32_t m3x_merkleize_validators_dev(m3x_ctx *ctx, const void *ssz_dev,
                                     uint64_t n, uint8_t out_root[32]) {
  // List[Validator, 2^40]: depth-40 tree + mix_in_length(n)
  if (!ctx || n > (1ull << 40)) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint8_t *root_dev = root_slot(ctx);
  int32_t rc = validator_subtree_root(ctx, (const uint8_t *)ssz_dev, n, 40,
                                      root_dev + 32);
  if (rc != M3X_OK) return rc;
  launch_finalize(ctx, root_dev + 32, 40, 40, (int64_t)n, root_dev);
  return read_root(ctx, root_dev, out_root);
}

int32_t m3x_merkleize_validators(m3x_ctx *ctx, const uint8_t *ssz, uint64_t n,
                                 uint8_t out_root[32]) {
  if (!ctx) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  DevTemps tmp(ctx->stream);
  const uint8_t *dev = n ? upload_validators(tmp, ssz, n) : nullptr;
  if (n && !dev) return M3X_ERR_HIP;
  return m3x_merkleize_validators_dev(ctx, dev, n, out_root);
}

int32_t m3x_merkleize_batch(m3x_ctx *ctx, const uint8_t *chunks,
                            const uint32_t *offsets, uint64_t n_elems,
                            uint8_t *out_roots) {
  if (!ctx || !offsets || n_elems == 0) return M3X_ERR_ARG;
  // the kernel folds a group in a private node[32][8]: every count must be
  // 0..32, so the offsets must not decrease either
  for (uint64_t i = 0; i < n_elems; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 32)
      return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint64_t in_bytes = (uint64_t)offsets[n_elems] * 32;
  uint64_t off_bytes = (n_elems + 1) * 4;
  uint64_t out_bytes = n_elems * 32;
  uint64_t need = in_bytes + off_bytes + out_bytes + 256;
  DevTemps tmp(ctx->stream);
  uint8_t *base =
      need <= m3x_ctx::SMALL_POOL_IN ? ctx->small_pool : tmp.alloc(need);
  if (!base) return M3X_ERR_HIP;
  uint8_t *in_d = base;
  uint8_t *off_d = base + in_bytes;
  uint8_t *out_d = base + in_bytes + ((off_bytes + 31) & ~31ull);
  bool queued = (!in_bytes || hipMemcpyAsync(in_d, chunks, in_bytes,
                                             hipMemcpyHostToDevice,
                                             ctx->stream) == hipSuccess) &&
                hipMemcpyAsync(off_d, offsets, off_bytes,
                               hipMemcpyHostToDevice,
                               ctx->stream) == hipSuccess;
  if (queued) {
    uint32_t blocks = (uint32_t)((n_elems + 63) / 64);
    hipLaunchKernelGGL(k_merkleize_batch, dim3(blocks), dim3(64), 0,
                       ctx->stream, in_d, (const uint32_t *)off_d, n_elems,
                       ctx->zeros_dev, out_d);
    tmp.download(out_roots, out_d, out_bytes);
  }
  // on failure too: nothing is freed while the stream may still use it
  return tmp.sync() && queued ? M3X_OK : M3X_ERR_HIP;
}

} // extern "C"

// ------------------- incremental registry merkleize --------
// The cache stores all tree levels contiguously in HBM (level l at node
// cache_level_off(cap_log2, l), cap>>l nodes). Updates rehash dirty leaves +
// root paths only (identical concurrent writes to a shared parent are
// benign).

struct m3x_registry_cache {
  uint32_t cap_log2 = 0;
  uint64_t capacity = 0;
  uint64_t n = 0; // current list length (mix_in_length)
  uint8_t *levels = nullptr;   // cache_level_off(cap_log2, cap_log2 + 1) nodes
  uint64_t *dirty_a = nullptr; // ping-pong dirty index lists
  uint64_t *dirty_b = nullptr;
  uint8_t *recs = nullptr;     // staging for update records
  uint64_t recs_cap = 0;
};

namespace {

// first node of level l: the counts of levels < l sum to 2cap - (2cap >> l)
__host__ __device__ inline uint64_t cache_level_off(uint32_t cap_log2,
                                                    uint32_t l) {
  uint64_t two_cap = 2ull << cap_log2;
  return two_cap - (two_cap >> l);
}

// hash one level range into the next (full build)
__global__ void k_cache_level(const uint8_t *__restrict__ src, uint64_t n_out,
                              uint8_t *__restrict__ dst) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  hash_pair(src + 64 * i, dst + 32 * i);
}

// recompute leaf roots for m dirty records and scatter into level 0
__global__ void k_cache_update_leaves(const uint8_t *__restrict__ recs,
                                      const uint64_t *__restrict__ idx,
                                      uint64_t m, uint8_t *__restrict__ level0) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint32_t root[8];
  validator_leaf_root(recs + 121 * t, root);
  store_node(level0 + 32 * idx[t], root);
}

// one propagation step: for each dirty node at level l, recompute its
// parent at level l+1 and emit the parent index
__global__ void k_cache_propagate(uint8_t *__restrict__ levels,
                                  uint32_t cap_log2, uint32_t l,
                                  const uint64_t *__restrict__ dirty,
                                  uint64_t m,
                                  uint64_t *__restrict__ dirty_next) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint64_t parent = dirty[t] >> 1;
  hash_pair(levels + 32 * (cache_level_off(cap_log2, l) + (parent << 1)),
            levels + 32 * (cache_level_off(cap_log2, l + 1) + parent));
  dirty_next[t] = parent;
}

} // namespace

extern "C" {

void m3x_registry_cache_destroy(m3x_registry_cache *c) {
  if (!c) return;
  if (c->levels) (void)hipFree(c->levels);
  if (c->dirty_a) (void)hipFree(c->dirty_a);
  if (c->dirty_b) (void)hipFree(c->dirty_b);
  if (c->recs) (void)hipFree(c->recs);
  delete c;
}

int32_t m3x_registry_cache_create(m3x_ctx *ctx, const uint8_t *ssz,
                                  uint64_t n, m3x_registry_cache **out) {
  if (!ctx || !out || n > (1ull << 24)) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  // destroyed on every return but the last
  std::unique_ptr<m3x_registry_cache, decltype(&m3x_registry_cache_destroy)> c(
      new m3x_registry_cache(), m3x_registry_cache_destroy);
  uint64_t cap = 256;
  uint32_t cl = 8;
  while (cap < n) {
    cap <<= 1;
    cl++;
  }
  c->cap_log2 = cl;
  c->capacity = cap;
  c->n = n;
  // the tree, and the dirty lists (record staging is grown on demand)
  if (hipMalloc(&c->levels, cache_level_off(cl, cl + 1) * 32) != hipSuccess ||
      hipMalloc(&c->dirty_a, 65536 * 8) != hipSuccess ||
      hipMalloc(&c->dirty_b, 65536 * 8) != hipSuccess)
    return M3X_ERR_NOMEM;
  DevTemps tmp(ctx->stream);
  const uint8_t *ssz_d = n ? upload_validators(tmp, ssz, n) : nullptr;
  if (n && !ssz_d) return M3X_ERR_HIP;
  // level 0: leaf roots for [0,n) then zero-ladder Z[0] (= zero chunk) pad
  M3X_HIP_CHECK(hipMemsetAsync(c->levels, 0, cap * 32, ctx->stream));
  if (n) launch_leaves(ctx, ssz_d, n, c->levels);
  // build all levels (full capacity, zero-padded leaves make the ladder)
  for (uint32_t l = 0; l < cl; l++) {
    uint64_t n_out = cap >> (l + 1);
    uint32_t blocks = (uint32_t)((n_out + 255) / 256);
    hipLaunchKernelGGL(k_cache_level, dim3(blocks), dim3(256), 0, ctx->stream,
                       c->levels + 32 * cache_level_off(cl, l), n_out,
                       c->levels + 32 * cache_level_off(cl, l + 1));
  }
  // the upload is freed on return: the build must have finished with it
  if (!tmp.sync()) return M3X_ERR_HIP;
  *out = c.release();
  return M3X_OK;
}

int32_t m3x_registry_cache_root(m3x_ctx *ctx, m3x_registry_cache *c,
                                uint8_t out_root[32]) {
  if (!ctx || !c) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  launch_finalize(ctx,
                  c->levels + 32 * cache_level_off(c->cap_log2, c->cap_log2),
                  c->cap_log2, 40, (int64_t)c->n, root_slot(ctx));
  return read_root(ctx, root_slot(ctx), out_root);
}

int32_t m3x_registry_cache_update(m3x_ctx *ctx, m3x_registry_cache *c,
                                  const uint64_t *indices,
                                  const uint8_t *recs, uint64_t m,
                                  uint8_t out_root[32]) {
  if (!ctx || !c) return M3X_ERR_ARG;
  if (m > 65536) return M3X_ERR_ARG; // dirty-list capacity this round
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  if (m) {
    // validate every index before anything changes: a rejected call leaves
    // the cache (its length included) as it was
    uint64_t new_n = c->n;
    for (uint64_t i = 0; i < m; i++) {
      if (indices[i] >= c->capacity) return M3X_ERR_ARG;
      if (indices[i] + 1 > new_n) new_n = indices[i] + 1;
    }
    uint64_t need = m * 121;
    if (c->recs_cap < need) {
      if (c->recs) (void)hipFree(c->recs);
      c->recs = nullptr;
      c->recs_cap = 0;
      if (hipMalloc(&c->recs, (need + 3) & ~3ull) != hipSuccess)
        return M3X_ERR_NOMEM;
      c->recs_cap = need;
    }
    M3X_HIP_CHECK(hipMemcpyAsync(c->recs, recs, m * 121,
                                 hipMemcpyHostToDevice, ctx->stream));
    M3X_HIP_CHECK(hipMemcpyAsync(c->dirty_a, indices, m * 8,
                                 hipMemcpyHostToDevice, ctx->stream));
    c->n = new_n;
    uint32_t blocks = (uint32_t)((m + 63) / 64);
    hipLaunchKernelGGL(k_cache_update_leaves, dim3(blocks), dim3(64), 0,
                       ctx->stream, c->recs, c->dirty_a, m, c->levels);
    uint64_t *cur = c->dirty_a, *nxt = c->dirty_b;
    for (uint32_t l = 0; l < c->cap_log2; l++) {
      hipLaunchKernelGGL(k_cache_propagate, dim3(blocks), dim3(64), 0,
                         ctx->stream, c->levels, c->cap_log2, l, cur, m, nxt);
      uint64_t *t = cur;
      cur = nxt;
      nxt = t;
    }
  }
  return m3x_registry_cache_root(ctx, c, out_root);
}

} // extern "C"
