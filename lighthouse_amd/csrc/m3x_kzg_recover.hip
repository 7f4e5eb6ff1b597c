// MI355X-native PeerDAS cell recovery (Fulu polynomial-commitments-sampling.md
// recover_polynomialcoeff and the cell half of recover_cells_and_kzg_proofs;
// Kzg::recover_all_cells, crypto/kzg/src/lib.rs:208-216): n blobs that share
// one set of k >= 64 known columns -> all 128 cells of each.
//
// A translation unit of its own, for the reason m3x_bls_each.hip records:
// the kernels of m3x_kzg_cells.hip keep compiling exactly as they did. The
// wave transform and the four-step row / column steps are shared with that
// file through kzg_ntt.hh; step 6 below is compute_cells' forward half, the
// same device functions.
//
// With M the missing cells, Z(x) = S(x^64), S(y) = prod_{c in M}
// (y - omega_128^bitrev7(c)), vanishes exactly on their cosets. E = the known
// evaluations (0 where missing), P = the blob polynomial: E Z = P Z on the
// whole 8192-point domain, and deg(P Z) < 8192, so
//   1 d  = IFFT_8192(E Z)                        = the coefficients of P Z
//   2 ce = FFT_8192(d_j 7^j)                     = P Z on the coset 7 <omega>
//   3 q  = ce / Z(7 omega^j)                     = P on that coset
//   4 Q  = IFFT_8192(q)_j 7^-j                   = the coefficients of P
//   5 Q[4096..8192) != 0: the cells lie on no polynomial of degree < 4096
//   6 cells = compute_cells' forward half of Q[0..4096)
// Z is never formed: x^64 is constant on a cell's coset, so Z takes one value
// per cell on the domain, S(omega_128^bitrev7(c)), and one per cell on the
// shifted domain, S'_c = S(7^64 omega_128^bitrev7(c)), never zero there. The
// product over all 128 roots is y^128 - 1, which on the shifted domain is the
// constant 7^8192 - 1, so 1 / S'_c is the product over the known cells by one
// constant: no inversion. That is 2 x 128 direct products, once per call
// (k_kzgr_vanish: one wave per cell, two roots per lane, a butterfly product),
// and each is a per-wave constant of the pass that uses it. The 1/8192 and
// 1/4096 of the inverse transforms are folded into the same two tables.
//
// An 8192-point transform is one radix-2 stage around two 4096-point
// four-step transforms, the identity compute_cells uses: the even-indexed
// evaluations (cells 0..63) are FFT_4096(lo + hi), the odd-indexed ones
// (cells 64..127) FFT_4096((lo - hi)_j omega_8192^j). A 128 x 64 split would
// need a 128-point wave transform, a second butterfly; here the radix-2 stage
// is one add and one subtract in the column kernels, which hold the two
// halves' elements of one index on one lane. Five passes over two staging
// arrays of 8192 fr per blob (2 x 256 KiB, L2-resident):
//   k_kzgr_rows   decode + canonical check, * S_c / 8192, inverse rows of
//                 both halves (128 waves per blob; a missing cell stores 0)
//   k_kzgr_shift  inverse columns of both halves -> lo, hi of P Z; * 7^j;
//                 radix-2 stage; forward rows of both halves (64 waves)
//   k_kzgr_quot   forward columns -> P Z on the coset, in cell order, which
//                 is the inverse rows' input order: * 1 / (4096 S'_c), inverse
//                 rows, without leaving the wave (128 waves)
//   k_kzgr_coef   inverse columns of both halves -> x = lo + hi, y = lo - hi
//                 of Q_j 7^j; hi == 0 <=> x == y, else the fail flag;
//                 * 7^-j; forward rows of both halves (64 waves)
//   k_kzgr_cells  forward columns, encode all 128 cells (128 waves)
// All 128 cells are written from the recovered polynomial; for a consistent
// input the known ones come out as they went in.
#include "fr_device.hh"
#include "kzg_cell_consts.h"
#include "kzg_ntt.hh"
#include "kzg_recover_consts.h"
#include "m3x_ctx.hh"
#include "../../include/m3x_consensus.h"

using namespace m3xf;

#define KZGC_CELLS 128
#define KZGC_CELL_BYTES 2048
#define KZGC_EXT_BYTES (KZGC_CELLS * KZGC_CELL_BYTES)
#define KZGC_MAX_BATCH 65535
#define KZGR_MISSING 0xffu

namespace {

// where cell c sits among the k known cells of a blob, or KZGR_MISSING
struct CellSlots {
  uint8_t slot[KZGC_CELLS];
};

// Wave c: the two values of Z that cell c's waves multiply by,
//   zs[c]   = S(y) / 8192,             y  = omega_128^bitrev7(c)
//   zinv[c] = 1 / (4096 S(y')) = prod_{known} (y' - root) / (4096 (7^8192 - 1)),
//                                      y' = 7^64 y
// Lane t takes the roots omega_128^t and omega_128^(t + 64) = -omega_128^t,
// those of cells m = bitrev7(t) and m + 1: a missing cell's factor goes into
// the first product, a known one's into the second, and the other product
// takes 1. Six xor steps multiply the 64 lanes' pairs, in a fixed order.
__global__ __launch_bounds__(64) void k_kzgr_vanish(uint64_t miss_lo,
                                                    uint64_t miss_hi,
                                                    fr *__restrict__ zs,
                                                    fr *__restrict__ zinv) {
  uint32_t c = blockIdx.x, t = threadIdx.x;
  fr w128, y, yc, root, nroot, one, f, g, s, sc;
  FRC_LOAD(w128, FRR_OMEGA128_MONT);
  fr_pow_u32(y, w128, bitrev_lo(c, 7));
  FRC_LOAD(f, FRR_SHIFT_POW64_MONT);
  fr_mul(yc, y, f);
  fr_pow_u32(root, w128, t);
  fr_neg(nroot, root);
  fr_one(one);
  uint32_t m = bitrev_lo(t, 7); // even: m and m + 1 sit in the same mask word
  uint64_t word = (m < 64 ? miss_lo : miss_hi) >> (m & 63);
  bool miss0 = (word & 1) != 0, miss1 = (word & 2) != 0;
  fr_sub(f, y, root);
  fr_select(s, miss0, f, one);
  fr_sub(f, y, nroot);
  fr_select(g, miss1, f, one);
  fr_mul(s, s, g);
  fr_sub(f, yc, root);
  fr_select(sc, miss0, one, f);
  fr_sub(f, yc, nroot);
  fr_select(g, miss1, one, f);
  fr_mul(sc, sc, g);
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    fr_shfl_xor(f, s, mask);
    fr_mul(s, s, f);
    fr_shfl_xor(g, sc, mask);
    fr_mul(sc, sc, g);
  }
  FRC_LOAD(f, FRR_INV8192_MONT);
  fr_mul(s, s, f);
  FRC_LOAD(f, FRR_QUOT_SCALE_MONT);
  fr_mul(sc, sc, f);
  if (t == 0) {
    zs[c] = s;
    zinv[c] = sc;
  }
}

// Wave (blob, cell cc = 64 h + c): half h's inverse row n2 = bitrev6(c) of
// E Z / 8192, t1[h][k1 * 64 + c]. Z is the constant zs[cc] on the cell.
__global__ __launch_bounds__(256) void k_kzgr_rows(
    const uint8_t *__restrict__ cells, uint64_t k, uint64_t n, CellSlots map,
    const fr *__restrict__ zs, fr *__restrict__ t1, int *__restrict__ fail) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 7;
  uint32_t cc = (uint32_t)wv & 127, c = cc & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr *dst = t1 + (2 * b + (cc >> 6)) * KZG_N + l * 64 + c;
  uint32_t slot = map.slot[cc];
  fr a;
  if (slot == KZGR_MISSING) { // wave-uniform: the transform of a zero row
    fr_zero(a);
    *dst = a;
    return;
  }
  const uint8_t *src = cells + ((b * k + slot) * 64 + l) * 32;
  uint32_t s[8];
  fr_limbs_from_be32(s, src);
  if (fr_ge_r(s)) { // non-canonical element: the call fails
    atomicOr(fail, 1);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = 0;
  }
  fr_from_std(a, s);
  kzgc_inv_row(a, c, l);
  fr_mul(a, a, zs[cc]);
  *dst = a;
}

// Inverse columns k1 of both halves: lane l ends with x = lo + hi and
// y = lo - hi of the transformed polynomial's coefficients j = k1 + 64 l and
// j + 4096 (y after its omega_8192^-j).
__device__ __forceinline__ void kzgr_inv_cols(fr &x, fr &y,
                                              const fr *__restrict__ t1,
                                              uint64_t b, uint32_t k1,
                                              uint32_t l) {
  const fr *src = t1 + 2 * b * KZG_N + k1 * 64 + l;
  fr w, tw;
  x = src[0];
  y = src[KZG_N];
  fr_ntt64_wave<false, true>(x, (int)l);
  fr_ntt64_wave<false, true>(y, (int)l);
  FRC_LOAD(w, FRC_OMEGA8192_INV_MONT);
  fr_pow_u32(tw, w, k1 + 64 * l);
  fr_mul(y, y, tw);
}

// Forward rows k1 of both halves, from the even half's input x and the odd
// half's y (before its omega_8192^j): t2[h][l * 64 + k1].
__device__ __forceinline__ void kzgr_fwd_rows(fr &x, fr &y,
                                              fr *__restrict__ t2, uint64_t b,
                                              uint32_t k1, uint32_t l) {
  fr *dst = t2 + 2 * b * KZG_N + l * 64 + k1;
  kzgc_fwd_row<false>(x, k1, l);
  kzgc_fwd_row<true>(y, k1, l);
  dst[0] = x;
  dst[KZG_N] = y;
}

// Wave (blob, k1): d = P Z's coefficients, d'_j = d_j 7^j, and the radix-2
// stage of FFT_8192(d'): lo' + hi' feeds the even half, lo' - hi' the odd.
__global__ __launch_bounds__(256) void k_kzgr_shift(const fr *__restrict__ t1,
                                                    uint64_t n,
                                                    fr *__restrict__ t2) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t k1 = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr x, y, lo, hi, w, tw;
  kzgr_inv_cols(x, y, t1, b, k1, l);
  fr_add(lo, x, y); // the 1/2 is in zs
  fr_sub(hi, x, y);
  FRC_LOAD(w, FRR_SHIFT_MONT);
  fr_pow_u32(tw, w, k1 + 64 * l);
  fr_mul(lo, lo, tw);
  fr_mul(hi, hi, tw);
  FRC_LOAD(w, FRR_SHIFT_POW4096_MONT);
  fr_mul(hi, hi, w);
  fr_add(x, lo, hi);
  fr_sub(y, lo, hi);
  kzgr_fwd_rows(x, y, t2, b, k1, l);
}

// Wave (blob, cell cc): the forward column leaves P Z on the shifted coset
// of cell cc, element i on lane i, which is the order the inverse row reads.
__global__ __launch_bounds__(256) void k_kzgr_quot(const fr *__restrict__ t2,
                                                   uint64_t n,
                                                   const fr *__restrict__ zinv,
                                                   fr *__restrict__ t1) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 7;
  uint32_t cc = (uint32_t)wv & 127, c = cc & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  uint64_t half = (2 * b + (cc >> 6)) * KZG_N;
  fr a = t2[half + c * 64 + l];
  fr_ntt64_wave<true, false>(a, (int)l);
  kzgc_inv_row(a, c, l);
  fr_mul(a, a, zinv[cc]);
  t1[half + l * 64 + c] = a;
}

// Wave (blob, k1): Q'_j = Q_j 7^j. Its upper half is zero exactly when
// x == y, and then Q_j = x 7^-j feeds both forward halves as in compute_cells.
__global__ __launch_bounds__(256) void k_kzgr_coef(const fr *__restrict__ t1,
                                                   uint64_t n,
                                                   fr *__restrict__ t2,
                                                   int *__restrict__ fail) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t k1 = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr x, y, w, tw;
  kzgr_inv_cols(x, y, t1, b, k1, l);
  if (!fr_eq(x, y)) atomicOr(fail, 1); // degree >= 4096: inconsistent cells
  FRC_LOAD(w, FRR_SHIFT_INV_MONT);
  fr_pow_u32(tw, w, k1 + 64 * l);
  fr_mul(x, x, tw);
  y = x;
  kzgr_fwd_rows(x, y, t2, b, k1, l);
}

// Wave (blob, cell cc): forward column, encode cell cc.
__global__ __launch_bounds__(256) void k_kzgr_cells(const fr *__restrict__ t2,
                                                    uint64_t n,
                                                    uint8_t *__restrict__ out) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 7;
  uint32_t cc = (uint32_t)wv & 127, c = cc & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr a = t2[(2 * b + (cc >> 6)) * KZG_N + c * 64 + l];
  kzgc_fwd_col_store(a, l, out + b * KZGC_EXT_BYTES + (64 * cc + l) * 32);
}

struct RecoverWork {
  fr *t1, *t2;   // [n*8192] each: [blob][half][4096]
  fr *zs, *zinv; // [128] each, by cell
  int *fail;     // [1]
};

int recover_layout(m3x_ctx *ctx, uint64_t n, RecoverWork &w) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.t1 = c.take<fr>(n * 2 * KZG_N);
        w.t2 = c.take<fr>(n * 2 * KZG_N);
        w.zs = c.take<fr>(KZGC_CELLS);
        w.zinv = c.take<fr>(KZGC_CELLS);
        w.fail = c.take<int>(1);
      });
}

// the checks made before anything is launched; fills the slot map and the
// missing-cell mask
bool recover_args_ok(const uint64_t *cell_ids, uint64_t k, uint64_t n,
                     CellSlots &map, uint64_t miss[2]) {
  if (!cell_ids || k < KZGC_CELLS / 2 || k > KZGC_CELLS || n > KZGC_MAX_BATCH)
    return false;
  for (int c = 0; c < KZGC_CELLS; c++) map.slot[c] = KZGR_MISSING;
  miss[0] = miss[1] = ~0ull;
  for (uint64_t t = 0; t < k; t++) {
    uint64_t c = cell_ids[t];
    if (c >= KZGC_CELLS || map.slot[c] != KZGR_MISSING) return false;
    map.slot[c] = (uint8_t)t;
    miss[c >> 6] &= ~(1ull << (c & 63));
  }
  return true;
}

} // namespace

extern "C" {

int32_t m3x_kzgc_recover_cells_dev(m3x_ctx *ctx, const uint64_t *cell_ids,
                                  uint64_t k, const void *cells_dev,
                                  uint64_t n, void *cells_out_dev) {
  CellSlots map;
  uint64_t miss[2];
  if (!ctx || !recover_args_ok(cell_ids, k, n, map, miss)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!cells_dev || !cells_out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  RecoverWork w;
  int rc = recover_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  hipStream_t st = ctx->stream;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, st));
  // 4 waves per block: 128 waves per blob in the row / column-of-cells
  // passes, 64 where one wave carries both halves; every wave is full
  dim3 per_cell((uint32_t)(n * 32)), per_index((uint32_t)(n * 16)), block(256);
  m3x::time_begin(ctx, M3X_K_KZGC_RECOVER);
  hipLaunchKernelGGL(k_kzgr_vanish, dim3(KZGC_CELLS), dim3(64), 0, st, miss[0],
                     miss[1], w.zs, w.zinv);
  hipLaunchKernelGGL(k_kzgr_rows, per_cell, block, 0, st,
                     (const uint8_t *)cells_dev, k, n, map, w.zs, w.t1, w.fail);
  hipLaunchKernelGGL(k_kzgr_shift, per_index, block, 0, st, w.t1, n, w.t2);
  hipLaunchKernelGGL(k_kzgr_quot, per_cell, block, 0, st, w.t2, n, w.zinv,
                     w.t1);
  hipLaunchKernelGGL(k_kzgr_coef, per_index, block, 0, st, w.t1, n, w.t2,
                     w.fail);
  hipLaunchKernelGGL(k_kzgr_cells, per_cell, block, 0, st, w.t2, n,
                     (uint8_t *)cells_out_dev);
  m3x::time_end(ctx, M3X_K_KZGC_RECOVER);
  int32_t fail = 1;
  M3X_HIP_CHECK(
      hipMemcpyAsync(&fail, w.fail, 4, hipMemcpyDeviceToHost, st));
  M3X_HIP_CHECK(hipStreamSynchronize(st));
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

int32_t m3x_kzgc_recover_cells(m3x_ctx *ctx, const uint64_t *cell_ids,
                              uint64_t k, const uint8_t *cells, uint64_t n,
                              uint8_t *cells_out) {
  CellSlots map;
  uint64_t miss[2];
  if (!ctx || !recover_args_ok(cell_ids, k, n, map, miss)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!cells || !cells_out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *in_d = tmp.upload(cells, n * k * KZGC_CELL_BYTES);
  uint8_t *out_d = tmp.alloc(n * KZGC_EXT_BYTES);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t rc = m3x_kzgc_recover_cells_dev(ctx, cell_ids, k, in_d, n, out_d);
  if (rc != M3X_OK) return rc;
  tmp.download(cells_out, out_d, n * KZGC_EXT_BYTES);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

} // extern "C"
