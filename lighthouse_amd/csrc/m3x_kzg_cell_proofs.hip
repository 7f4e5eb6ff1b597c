// MI355X-native PeerDAS cell proofs (Fulu polynomial-commitments-sampling.md
// compute_cells_and_kzg_proofs / recover_cells_and_kzg_proofs; the proof half
// of Kzg::compute_cells_and_proofs, crypto/kzg/src/lib.rs:171-185).
//
// A translation unit of its own, for the reason m3x_bls_each.hip records: the
// kernels of m3x_kzg.hip, m3x_kzg_cells.hip and m3x_kzg_recover.hip keep
// compiling exactly as they did. The table build (k_kzgp_bases, k_kzgp_table)
// is reached through launchers of m3x_kzg.hh, the transforms come from
// kzg_ntt.hh.
//
// p = the blob's coefficient list, y_c = h_c^64 = omega_128^bitrev7(c). The
// proof of cell c is [q_c(tau)]G1, q_c = p // (X^64 - y_c), and
// q_c[j] = sum_{m>=0} p[j + 64(m+1)] y_c^m, so with
//   h_m     = sum_{j=0}^{4095-64(m+1)} p[j + 64(m+1)] g1_monomial[j]  m = 0..62
//   proof_c = sum_{m=0}^{62} y_c^m h_m                                c = 0..127
// the proofs are a 128-point G1 transform of h_0..h_62 padded with infinity.
//
// Stage 1, all fixed-base: the 63 sums h_m straight from a table over
// g1_monomial, k_kzgp_msm's scheme (signed 4-bit digits, look-ups joined by
// mixed additions, no doublings, an LDS tree per block). 129 024 table terms
// per blob, no serial chain.
//   k_kzgcp_rows      canonical check, inverse rows (kzgc_inv_row)
//   k_kzgcp_digits    inverse columns -> coefficients, stored as the 64
//                     signed digits of each (what the look-ups read)
//   k_kzgcp_toeplitz  block (64 values of j, m): 16 look-ups per lane
//   k_kzgcp_join      the <= 63 block sums of each (blob, m)
// Stage 2, one wave per blob, the 128 points in LDS:
//   k_kzgcp_dft       radix-2 decimation in frequency: natural-order input,
//                     after each subtraction a multiplication by
//                     omega_128^(i * 64 / span), frequency bitrev7(c) at
//                     position c, which is cell order
//   k_kzgcp_compress  one lane per proof
#include "bls_device.hh"
#include "fr_device.hh"
#include "kzg_cell_consts.h"
#include "kzg_cell_proof_consts.h"
#include "kzg_ntt.hh"
#include "m3x_ctx.hh"
#include "m3x_kzg.hh"
#include "../../include/m3x_consensus.h"
#include <new>

using namespace m3xb;
using namespace m3xf;

#define KZG_BLOB_BYTES 131072
#define KZGC_CELLS 128
#define KZGC_EXT_BYTES (KZGC_CELLS * 2048) // one blob's cells
#define KZGC_MAX_BATCH 65535
#define KZGCP_SUMS 63                      // h_0..h_62
#define KZGCP_BLOCKS (KZGCP_SUMS * (KZGCP_SUMS + 1) / 2) // 2016 per blob
#define KZGCP_PER_LANE 16                  // windows (look-ups) per lane

namespace {

// first block sum of h_m: sums 0..m-1 have 63, 62, ... blocks
__device__ __forceinline__ uint32_t kzgcp_first_block(uint32_t m) {
  return KZGCP_SUMS * m - m * (m - 1) / 2;
}

// --------------------------------------------------- stage 1: coefficients

// k_kzgc_rows without the cell copy; blob b starts at blobs + b * stride, so
// the recovered blobs are read in place inside their cells.
// t1[k1 * 64 + c] = A[n2][k1] * omega_4096^(-n2 k1) / 4096.
__global__ __launch_bounds__(256) void k_kzgcp_rows(
    const uint8_t *__restrict__ blobs, uint64_t stride, uint64_t n,
    fr *__restrict__ t1, int *__restrict__ fail) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t c = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  const uint8_t *src = blobs + b * stride + (64 * c + l) * 32;
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[7 - i] = ld_be32(src + 4 * i);
  if (fr_ge_r(s)) { // non-canonical element: the call fails
    atomicOr(fail, 1);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = 0;
  }
  fr a, w;
  fr_from_std(a, s);
  kzgc_inv_row(a, c, l);
  FRC_LOAD(w, FR_N_INV_MONT);
  fr_mul(a, a, w);
  t1[b * KZG_N + l * 64 + c] = a;
}

// Wave (blob, k1): the inverse column gives coefficient i = k1 + 64 l on lane
// l (k_kzgc_mid's first step). Stored as its 64 signed digits, one byte each:
// s = sum_k d_k 16^k, d_k in [-7, 8]; d = nibble + carry, d > 8 => d - 16 and
// carry 1. A coefficient is < r < 2^255: the top nibble is <= 7 and never
// carries out.
__global__ __launch_bounds__(256) void k_kzgcp_digits(
    const fr *__restrict__ t1, uint64_t n, uint32_t *__restrict__ dig) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t k1 = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr a = t1[b * KZG_N + k1 * 64 + l];
  fr_ntt64_wave<false, true>(a, (int)l);
  uint32_t s[8];
  fr_to_std(s, a);
  uint32_t *dst = dig + (b * KZG_N + k1 + 64 * l) * (KZGP_WINDOWS / 4);
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      int d = (int)((s[i] >> (4 * k)) & 15) + (int)carry;
      carry = d > 8 ? 1u : 0u;
      if (carry) d -= 16;
      w[k >> 2] |= ((uint32_t)d & 0xffu) << (8 * (k & 3));
    }
    dst[2 * i] = w[0];
    dst[2 * i + 1] = w[1];
  }
}

// ----------------------------------------------------- stage 1: the sums

// Block (bx, m, blob): the terms j = 64 bx .. 64 bx + 63 of h_m, lane
// (j, quarter q) owning windows 16q..16q+15 of p[j + 64(m+1)]. h_m runs over
// j < 4096 - 64(m+1) = 64 (63 - m): block edges fall on the sum's range, the
// blocks with bx + m > 62 return at once, and i <= 64 * 62 + 127 = 4095.
// Every addition takes the doubling, inverse and infinity branches of
// g1j_add / g1j_add_aff.
__global__ __launch_bounds__(256) void k_kzgcp_toeplitz(
    const uint32_t *__restrict__ dig, const g1t *__restrict__ table,
    g1j *__restrict__ partial) {
  __shared__ g1j lds[256];
  uint32_t bx = blockIdx.x, m = blockIdx.y, t = threadIdx.x;
  uint64_t blob = blockIdx.z;
  if (bx + m >= KZGCP_SUMS) return; // block-uniform
  uint32_t j = 64 * bx + (t >> 2), q = t & 3;
  uint32_t i = j + 64 * (m + 1);
  const uint4 dv = *reinterpret_cast<const uint4 *>(
      dig + (blob * KZG_N + i) * (KZGP_WINDOWS / 4) + 4 * q);
  const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
  g1j acc;
  g1j_set_inf(acc);
  for (uint32_t k = 0; k < KZGCP_PER_LANE; k++) {
    int d = (int)(int8_t)(dw[k >> 2] >> (8 * (k & 3)));
    if (d == 0) continue;
    uint32_t mag = (uint32_t)(d < 0 ? -d : d); // 1..8
    uint32_t win = KZGCP_PER_LANE * q + k;
    const g1t &tp = table[((uint64_t)win * KZG_N + j) * KZGP_DIGITS + (mag - 1)];
    g1a pt;
    pt.x = tp.x;
    pt.y = tp.y;
    pt.inf = 0;
    if (d < 0) fp_neg(pt.y, pt.y);
    g1j_add_aff(acc, acc, pt);
  }
  lds[t] = acc;
  block_tree_reduce<g1j, 256>(lds, (int)t, g1j_add_op{});
  if (t == 0)
    partial[blob * KZGCP_BLOCKS + kzgcp_first_block(m) + bx] = lds[0];
}

// block (m, blob): h_m = the 63 - m block sums
__global__ __launch_bounds__(64) void k_kzgcp_join(
    const g1j *__restrict__ partial, g1j *__restrict__ hs) {
  __shared__ g1j lds[64];
  uint32_t m = blockIdx.x, t = threadIdx.x;
  uint64_t blob = blockIdx.y;
  g1j v;
  if (t < KZGCP_SUMS - m)
    v = partial[blob * KZGCP_BLOCKS + kzgcp_first_block(m) + t];
  else
    g1j_set_inf(v);
  lds[t] = v;
  block_tree_reduce<g1j, 64>(lds, (int)t, g1j_add_op{});
  if (t == 0) hs[blob * KZGCP_SUMS + m] = lds[0];
}

// ------------------------------------------------------- stage 2: the DFT

// p = [omega_128^k] p; k == 0 and infinity do not multiply. The windowed form
// of g1_mul_be32_aff's chain: the lanes of a wave hold different twiddles, so
// a bit-by-bit chain pays an addition at nearly every bit; with [1..15] p
// tabulated per lane it is one addition per 4 doublings, and the base stays
// Jacobian (no inversion). Every addition is g1j_add, with its doubling,
// inverse and infinity branches.
__device__ inline void kzgcp_twiddle(g1j &p, uint32_t k) {
  if (k == 0 || g1j_is_inf(p)) return;
  g1j tab[15]; // tab[d - 1] = [d] p
  tab[0] = p;
#pragma unroll 1
  for (int d = 2; d <= 15; d++) {
    if (d & 1)
      g1j_add(tab[d - 1], tab[d - 2], p);
    else
      g1j_dbl(tab[d - 1], tab[d / 2 - 1]);
  }
  const uint8_t *be = FRP_W128_BE[k];
  g1j acc;
  g1j_set_inf(acc);
#pragma unroll 1
  for (int i = 0; i < 64; i++) {
    for (int b = 0; b < 4; b++) g1j_dbl(acc, acc);
    uint32_t d = (be[i >> 1] >> ((i & 1) ? 0 : 4)) & 15;
    if (d) g1j_add(acc, acc, tab[d - 1]);
  }
  p = acc;
}

// One wave per blob, lane t one butterfly of each of the 7 stages. The first
// stage's upper inputs are all infinity: it is the copy and the twiddle. The
// last stage's twiddles are all 1: it does not multiply.
__global__ __launch_bounds__(64, 1) void k_kzgcp_dft(
    const g1j *__restrict__ hs, g1j *__restrict__ pts) {
  __shared__ g1j P[KZGC_CELLS];
  uint32_t t = threadIdx.x;
  uint64_t blob = blockIdx.x;
  {
    g1j a;
    if (t < KZGCP_SUMS)
      a = hs[blob * KZGCP_SUMS + t];
    else
      g1j_set_inf(a);
    P[t] = a;
    kzgcp_twiddle(a, t);
    P[t + 64] = a;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t half = 32; half >= 1; half >>= 1) {
    uint32_t pos = t & (half - 1);
    uint32_t lo = 2 * (t - pos) + pos, hi = lo + half;
    g1j x = P[lo], y = P[hi], sum;
    g1j_add(sum, x, y);
    fp_neg(y.y, y.y);
    g1j_add(x, x, y);
    if (half > 1) kzgcp_twiddle(x, pos * (64 / half));
    P[lo] = sum;
    P[hi] = x;
    __syncthreads();
  }
  pts[blob * KZGC_CELLS + t] = P[t];
  pts[blob * KZGC_CELLS + 64 + t] = P[t + 64];
}

// one lane per proof; infinity encodes as 0xc0 00...
__global__ __launch_bounds__(64, 1) void k_kzgcp_compress(
    const g1j *__restrict__ pts, uint64_t count, uint8_t *__restrict__ out) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= count) return;
  g1_compress(out + 48 * lane, pts[lane]);
}

// ------------------------------------------------------------------- host

struct ProofWork {
  fr *t1;        // [n*4096] inverse rows
  uint32_t *dig; // [n*4096*16] signed digits of the coefficients, 4 a word
  g1j *partial;  // [n*2016] block sums of stage 1
  g1j *hs;       // [n*63] h_m
  g1j *pts;      // [n*128] the proofs before compression
  int *fail;     // [1]
};

int proofs_layout(m3x_ctx *ctx, uint64_t n, ProofWork &w) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.t1 = c.take<fr>(n * KZG_N);
        w.dig = c.take<uint32_t>(n * KZG_N * (KZGP_WINDOWS / 4));
        w.partial = c.take<g1j>(n * KZGCP_BLOCKS);
        w.hs = c.take<g1j>(n * KZGCP_SUMS);
        w.pts = c.take<g1j>(n * KZGC_CELLS);
        w.fail = c.take<int>(1);
      });
}

bool proofs_args_ok(m3x_ctx *ctx, m3x_kzg *kzg, uint64_t n) {
  return ctx && kzg && kzg->mono_table && kzg->device == ctx->device &&
         n <= KZGC_MAX_BATCH;
}

// The proof pipeline over n blobs in device memory, blob b at blobs_dev +
// b * stride. The caller holds ctx->mu and has set the device; n >= 1.
int32_t run_proofs(m3x_ctx *ctx, m3x_kzg *kzg, const uint8_t *blobs_dev,
                   uint64_t stride, uint64_t n, uint8_t *proofs_out_dev) {
  ProofWork w;
  int rc = proofs_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  hipStream_t st = ctx->stream;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, st));
  // 64 waves per blob and pass, 4 waves per block: every wave is full
  dim3 per_index((uint32_t)(n * 16)), block(256);
  m3x::time_begin(ctx, M3X_K_KZGC_TOEPLITZ);
  hipLaunchKernelGGL(k_kzgcp_rows, per_index, block, 0, st, blobs_dev, stride,
                     n, w.t1, w.fail);
  hipLaunchKernelGGL(k_kzgcp_digits, per_index, block, 0, st, w.t1, n, w.dig);
  hipLaunchKernelGGL(k_kzgcp_toeplitz,
                     dim3(KZGCP_SUMS, KZGCP_SUMS, (uint32_t)n), block, 0, st,
                     w.dig, kzg->mono_table, w.partial);
  hipLaunchKernelGGL(k_kzgcp_join, dim3(KZGCP_SUMS, (uint32_t)n), dim3(64), 0,
                     st, w.partial, w.hs);
  m3x::time_end(ctx, M3X_K_KZGC_TOEPLITZ);
  m3x::time_begin(ctx, M3X_K_KZGC_PROOF_DFT);
  hipLaunchKernelGGL(k_kzgcp_dft, dim3((uint32_t)n), dim3(64), 0, st, w.hs,
                     w.pts);
  hipLaunchKernelGGL(k_kzgcp_compress, dim3((uint32_t)(n * 2)), dim3(64), 0, st,
                     w.pts, n * KZGC_CELLS, proofs_out_dev);
  m3x::time_end(ctx, M3X_K_KZGC_PROOF_DFT);
  int32_t fail = 1;
  M3X_HIP_CHECK(hipMemcpyAsync(&fail, w.fail, 4, hipMemcpyDeviceToHost, st));
  M3X_HIP_CHECK(hipStreamSynchronize(st));
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

uint32_t bitrev12(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 12; i++) r |= ((v >> i) & 1u) << (11 - i);
  return r;
}

} // namespace

extern "C" {

int32_t m3x_kzgc_load_g1_monomial(m3x_ctx *ctx, m3x_kzg *kzg,
                                 const uint8_t *g1_monomial) {
  if (!ctx || !kzg || !kzg->g2 || kzg->device != ctx->device || !g1_monomial ||
      kzg->mono_table)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  // k_kzgp_bases reads entry bitrev12(e) for base e; bit reversal is an
  // involution, so the list uploaded pre-permuted gives natural order
  uint8_t *perm = new (std::nothrow) uint8_t[(uint64_t)KZG_N * 48];
  if (!perm) return M3X_ERR_NOMEM;
  for (uint32_t e = 0; e < KZG_N; e++)
    __builtin_memcpy(perm + 48 * (uint64_t)bitrev12(e), g1_monomial + 48 * (uint64_t)e, 48);
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *mono_d = tmp.upload(perm, (uint64_t)KZG_N * 48);
  delete[] perm;
  int *fail_d = tmp.alloc<int>(4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  g1j *bases = tmp.alloc<g1j>((uint64_t)KZGP_WINDOWS * KZG_N * sizeof(g1j));
  g1t *table = tmp.alloc<g1t>(KZGP_TABLE_POINTS * sizeof(g1t));
  if (!tmp.ok()) return M3X_ERR_NOMEM;
  M3X_HIP_CHECK(hipMemsetAsync(fail_d, 0, 4, ctx->stream));
  m3x::launch_kzgp_bases(ctx->stream, mono_d, bases, fail_d);
  int fail = 1;
  tmp.download(&fail, fail_d, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail) return M3X_ERR_ENCODING;
  m3x::launch_kzgp_table(ctx->stream, bases, table);
  if (!tmp.sync()) return M3X_ERR_HIP;
  kzg->mono_table = tmp.release(table); // the handle owns it from here
  return M3X_OK;
}

int32_t m3x_kzgc_compute_cells_and_proofs_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                             const void *blobs_dev, uint64_t n,
                                             void *cells_out_dev,
                                             void *proofs_out_dev) {
  if (!proofs_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs_dev || !proofs_out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  if (cells_out_dev) { // the cells are compute_cells' own, bit for bit
    int32_t rc = m3x_kzgc_compute_cells_dev(ctx, blobs_dev, n, cells_out_dev);
    if (rc != M3X_OK) return rc;
  }
  return run_proofs(ctx, kzg, (const uint8_t *)blobs_dev, KZG_BLOB_BYTES, n,
                    (uint8_t *)proofs_out_dev);
}

int32_t m3x_kzgc_compute_cells_and_proofs(m3x_ctx *ctx, m3x_kzg *kzg,
                                         const uint8_t *blobs, uint64_t n,
                                         uint8_t *cells_out,
                                         uint8_t *proofs_out) {
  if (!proofs_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs || !proofs_out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES);
  uint8_t *ce_d = cells_out ? tmp.alloc(n * KZGC_EXT_BYTES) : nullptr;
  uint8_t *pr_d = tmp.alloc(n * KZGC_CELLS * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t rc =
      m3x_kzgc_compute_cells_and_proofs_dev(ctx, kzg, bl_d, n, ce_d, pr_d);
  if (rc != M3X_OK) return rc;
  if (cells_out) tmp.download(cells_out, ce_d, n * KZGC_EXT_BYTES);
  tmp.download(proofs_out, pr_d, n * KZGC_CELLS * 48);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_kzgc_recover_cells_and_proofs_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                             const uint64_t *cell_ids,
                                             uint64_t k, const void *cells_dev,
                                             uint64_t n, void *cells_out_dev,
                                             void *proofs_out_dev) {
  // recovery's own rules first: its n == 0 form checks them and launches
  // nothing
  if (!ctx || n > KZGC_MAX_BATCH) return M3X_ERR_ARG;
  int32_t rc = m3x_kzgc_recover_cells_dev(ctx, cell_ids, k, nullptr, 0, nullptr);
  if (rc != M3X_OK) return rc;
  if (!proofs_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!cells_dev || !cells_out_dev || !proofs_out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  rc = m3x_kzgc_recover_cells_dev(ctx, cell_ids, k, cells_dev, n, cells_out_dev);
  if (rc != M3X_OK) return rc;
  // cells 0..63 of each output are the recovered blob: read in place
  return run_proofs(ctx, kzg, (const uint8_t *)cells_out_dev, KZGC_EXT_BYTES, n,
                    (uint8_t *)proofs_out_dev);
}

int32_t m3x_kzgc_recover_cells_and_proofs(m3x_ctx *ctx, m3x_kzg *kzg,
                                         const uint64_t *cell_ids, uint64_t k,
                                         const uint8_t *cells, uint64_t n,
                                         uint8_t *cells_out,
                                         uint8_t *proofs_out) {
  if (!ctx || n > KZGC_MAX_BATCH) return M3X_ERR_ARG;
  int32_t rc = m3x_kzgc_recover_cells_dev(ctx, cell_ids, k, nullptr, 0, nullptr);
  if (rc != M3X_OK) return rc;
  if (!proofs_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!cells || !cells_out || !proofs_out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *in_d = tmp.upload(cells, n * k * 2048);
  uint8_t *ce_d = tmp.alloc(n * KZGC_EXT_BYTES);
  uint8_t *pr_d = tmp.alloc(n * KZGC_CELLS * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  rc = m3x_kzgc_recover_cells_and_proofs_dev(ctx, kzg, cell_ids, k, in_d, n,
                                             ce_d, pr_d);
  if (rc != M3X_OK) return rc;
  tmp.download(cells_out, ce_d, n * KZGC_EXT_BYTES);
  tmp.download(proofs_out, pr_d, n * KZGC_CELLS * 48);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

} // extern "C"
