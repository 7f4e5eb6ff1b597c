// The wave-wide 64-point transform over Fr and the row / column steps of the
// 64 x 64 four-step 4096-point transforms built on it, shared by the cell
// pipeline (m3x_kzg_cells.hip) and cell recovery (m3x_kzg_recover.hip).
// Internal linkage: each translation unit inlines its own copy, and the cell
// kernels compile as they did when this code sat inside their file.
//
// fr_ntt64_wave is the core: a 64-point radix-2 transform, one element per
// lane, the six butterfly stages exchanged with __shfl_xor (no LDS).
// Decimation in time takes bit-reversed input to natural output, decimation
// in frequency the other way round, so no kernel permutes.
//
// Index conventions of the four-step passes, omega = omega_4096: an
// evaluation index is n = 64 n1 + n2, a coefficient index k = k1 + 64 k2.
// The staging arrays are transposed on the store, so every pass reads runs
// of 64 consecutive elements:
//   inverse rows     in: cell order (row n2 = bitrev6(c), bit-reversed)
//                    out: t1[k1 * 64 + c]
//   inverse columns  in: t1[k1 * 64 + l]; lane l ends with coefficient
//                    k1 + 64 l
//   forward rows     in: coefficient k1 + 64 l on lane l; out: t2[l * 64 + k1]
//   forward columns  in: t2[c * 64 + l]; lane i ends with element i of cell c
#pragma once
#include "fr_device.hh"
#include "kzg_cell_consts.h"

#define KZG_N 4096

namespace {

using m3xf::fr;

#define FRC_LOAD(dst, C)                                                       \
  do {                                                                         \
    _Pragma("unroll") for (int _i = 0; _i < 8; _i++)(dst).v[_i] = C[_i];       \
  } while (0)

__device__ __forceinline__ uint32_t bitrev_lo(uint32_t v, int bits) {
  return __builtin_bitreverse32(v) >> (32 - bits);
}

__device__ __forceinline__ void fr_pow_u32(fr &r, const fr &a, uint32_t e) {
  m3xf::fr_pow(r, a, &e, 1);
}

// every lane's partner value, lane ^ mask
__device__ __forceinline__ void fr_shfl_xor(fr &r, const fr &a, int mask) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_xor((int)a.v[i], mask, 64);
}

__device__ __forceinline__ void fr_select(fr &r, bool c, const fr &a,
                                          const fr &b) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
}

// 64-point transform across one full wave, lane l holding one element:
//   X[k] = sum_j x[j] * w^(jk),  w = omega_64 (INV: omega_64^-1, unscaled)
// DIF = false: lane l holds x[bitrev6(l)] on entry and X[l] on return
// DIF = true:  lane l holds x[l] on entry and X[bitrev6(l)] on return
// All 64 lanes must be active. Every lane multiplies and the result is
// selected: a branch would run both sides for the wave anyway.
template <bool DIF, bool INV>
__device__ __forceinline__ void fr_ntt64_wave(fr &a, int lane) {
  using namespace m3xf;
#pragma unroll
  for (int s = 0; s < 6; s++) {
    const int half = DIF ? (32 >> s) : (1 << s);
    const bool hi = (lane & half) != 0;
    uint32_t e = (uint32_t)(lane & (half - 1)) * (uint32_t)(32 / half);
    if (INV) e = (64 - e) & 63;
    fr tw, t, p, sum, dif;
    FRC_LOAD(tw, FRC_W64_MONT[e]);
    t = a;
    if (!DIF && half > 1) { // the upper input is twiddled before the butterfly
      fr m;
      fr_mul(m, a, tw);
      fr_select(t, hi, m, a);
    }
    fr_shfl_xor(p, t, half);
    fr_add(sum, t, p);
    fr_sub(dif, p, t);
    if (DIF && half > 1) fr_mul(dif, dif, tw); // ... or the lower output after
    fr_select(a, hi, dif, sum);
  }
}

__device__ __forceinline__ void st_be32(uint8_t *p, uint32_t v) {
  v = __builtin_bswap32(v);
  __builtin_memcpy(p, &v, 4);
}

// The wave a thread belongs to, out of 4 per block
__device__ __forceinline__ uint64_t wave_index() {
  return (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
}

// Inverse transform, row n2 = bitrev6(c): lane l holds the row's element
// n1 = bitrev6(l) on entry (cell order) and
// A[n2][k1 = l] * omega_4096^(-n2 k1) on return, unscaled.
__device__ __forceinline__ void kzgc_inv_row(fr &a, uint32_t c, uint32_t l) {
  fr w, tw;
  fr_ntt64_wave<false, true>(a, (int)l);
  FRC_LOAD(w, FRC_OMEGA4096_INV_MONT);
  fr_pow_u32(tw, w, bitrev_lo(c, 6) * l);
  m3xf::fr_mul(a, a, tw);
}

// Forward transform, row n2 = k1: lane l holds coefficient j = k1 + 64 l on
// entry. SHIFT scales it by omega_8192^j first, which turns the transform
// into the one over the odd 8192nd roots (cells 64..127). On return lane l
// holds B[k1][bitrev6(l)] * omega_4096^(k1 bitrev6(l)).
template <bool SHIFT>
__device__ __forceinline__ void kzgc_fwd_row(fr &a, uint32_t k1, uint32_t l) {
  fr w, tw;
  if (SHIFT) {
    FRC_LOAD(w, FRC_OMEGA8192_MONT);
    fr_pow_u32(tw, w, k1 + 64 * l);
    m3xf::fr_mul(a, a, tw);
  }
  fr_ntt64_wave<true, false>(a, (int)l);
  FRC_LOAD(w, FR_OMEGA_MONT);
  fr_pow_u32(tw, w, k1 * bitrev_lo(l, 6));
  m3xf::fr_mul(a, a, tw);
}

// Forward transform, column k1 = bitrev6(c) in natural order: lane i ends
// with F[bitrev6(c) + 64 bitrev6(i)] = F[bitrev12(64 c + i)], element i of
// the cell, and stores it at dst (32 bytes, canonical big-endian).
__device__ __forceinline__ void kzgc_fwd_col_store(fr &a, uint32_t l,
                                                   uint8_t *dst) {
  fr_ntt64_wave<true, false>(a, (int)l);
  uint32_t s[8];
  m3xf::fr_to_std(s, a);
#pragma unroll
  for (int i = 0; i < 8; i++) st_be32(dst + 4 * i, s[7 - i]);
}

} // namespace
