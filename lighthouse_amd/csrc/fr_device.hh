// BLS12-381 scalar field (Fr) device arithmetic for gfx950 — the field the
// Deneb KZG blob polynomials live in (m3x_kzg.hip).
//
// 255-bit Montgomery form with R = 2^256 on 8 x 32-bit limbs, the same
// CIOS shape as fp_mul in bls_device.hh: each inner multiply-accumulate is
// one v_mad_u64_u32 plus a 32-bit carry fold. r < 2^255, so a CIOS result
// is < 2r < 2^256 and the extra carry limb is always clear after the
// final shift; the conditional subtract only compares the 8 limbs.
//
// Constants come from kzg_consts.h (generated + numerically validated by
// tests/golden/gen_kzg_fixtures.py; constexpr so device code folds them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kzg_consts.h"

// function qualifier; a host build (CPU unit check of the limb code) may
// predefine it as `__host__ __device__ inline`
#ifndef M3X_FR_FN
#define M3X_FR_FN __device__ __forceinline__
#endif

namespace m3xf {

struct fr {
  uint32_t v[8];
}; // Montgomery form, little-endian limbs, always < r

M3X_FR_FN bool fr_ge_r(const uint32_t t[8]) {
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (t[i] > FR_MOD[i]) return true;
    if (t[i] < FR_MOD[i]) return false;
  }
  return true;
}

M3X_FR_FN void fr_sub_r(uint32_t t[8]) {
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t x = (uint64_t)t[i] - FR_MOD[i] - bw;
    t[i] = (uint32_t)x;
    bw = (x >> 32) & 1;
  }
}

M3X_FR_FN void fr_zero(fr &r) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
}

M3X_FR_FN void fr_one(fr &r) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = FR_ONE_MONT[i];
}

M3X_FR_FN bool fr_is_zero(const fr &a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}

M3X_FR_FN bool fr_eq(const fr &a, const fr &b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}

M3X_FR_FN void fr_add(fr &r, const fr &a, const fr &b) {
  uint64_t c = 0;
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  // a + b < 2r < 2^256: no carry out of the top limb
  if (fr_ge_r(t)) fr_sub_r(t);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
}

M3X_FR_FN void fr_sub(fr &r, const fr &a, const fr &b) {
  uint64_t bw = 0;
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t x = (uint64_t)a.v[i] - b.v[i] - bw;
    t[i] = (uint32_t)x;
    bw = (x >> 32) & 1;
  }
  if (bw) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)t[i] + FR_MOD[i];
      t[i] = (uint32_t)c;
      c >>= 32;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
}

M3X_FR_FN void fr_neg(fr &r, const fr &a) {
  fr z;
  fr_zero(z);
  fr_sub(r, z, a);
}

// Montgomery multiply, 8x32-bit limb CIOS (fp_mul's shape, 12 -> 8 limbs)
M3X_FR_FN void fr_mul(fr &r, const fr &a, const fr &b) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      uint64_t s = (uint64_t)a.v[j] * b.v[i] + t[j] + (uint32_t)c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    uint64_t s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    uint32_t m = t[0] * FR_N0;
    c = ((uint64_t)m * FR_MOD[0] + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      uint64_t s2 = (uint64_t)m * FR_MOD[j] + t[j] + (uint32_t)c;
      t[j - 1] = (uint32_t)s2;
      c = s2 >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
    t[9] = 0;
  }
  if (t[8] || fr_ge_r(t)) fr_sub_r(t);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
}

// 8x32 SOS squaring (fp_sqr's shape): 28 cross + 8 diagonal MACs + the
// 64-MAC Montgomery reduction = 100 MACs vs fr_mul's 128
M3X_FR_FN void fr_sqr(fr &r, const fr &a) {
  uint32_t t[17];
#pragma unroll
  for (int i = 0; i < 17; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 7; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = i + 1; j < 8; j++) {
      uint64_t p = (uint64_t)a.v[i] * a.v[j] + t[i + j] + (uint32_t)c;
      t[i + j] = (uint32_t)p;
      c = p >> 32;
    }
    t[i + 8] = (uint32_t)c;
  }
  uint32_t cc = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    uint32_t nv = (t[i] << 1) | cc;
    cc = t[i] >> 31;
    t[i] = nv;
  }
  {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t p = (uint64_t)a.v[i] * a.v[i] + t[2 * i] + (uint32_t)c;
      t[2 * i] = (uint32_t)p;
      uint64_t p2 = (uint64_t)t[2 * i + 1] + (p >> 32);
      t[2 * i + 1] = (uint32_t)p2;
      c = p2 >> 32;
    }
  }
  // Montgomery reduce the 16-limb square (< r^2 < r*2^256)
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = t[i];
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t m = w[0] * FR_N0;
    uint64_t c = ((uint64_t)m * FR_MOD[0] + w[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      uint64_t p = (uint64_t)m * FR_MOD[j] + w[j] + (uint32_t)c;
      w[j - 1] = (uint32_t)p;
      c = p >> 32;
    }
    uint64_t p = (uint64_t)t[8 + i] + c + carry;
    w[7] = (uint32_t)p;
    carry = (uint32_t)(p >> 32);
  }
  if (carry || fr_ge_r(w)) fr_sub_r(w);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
}

// standard-form limbs -> Montgomery (input must be < r)
M3X_FR_FN void fr_from_std(fr &r, const uint32_t s[8]) {
  fr a, r2;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    a.v[i] = s[i];
    r2.v[i] = FR_R2[i];
  }
  fr_mul(r, a, r2);
}

M3X_FR_FN void fr_to_std(uint32_t s[8], const fr &a) {
  fr one_std, t;
#pragma unroll
  for (int i = 0; i < 8; i++) one_std.v[i] = (i == 0) ? 1u : 0u;
  fr_mul(t, a, one_std);
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = t.v[i];
}

// 32-byte big-endian -> standard limbs (no range check)
M3X_FR_FN void fr_limbs_from_be32(uint32_t s[8], const uint8_t *b) {
#pragma unroll
  for (int i = 0; i < 8; i++)
    s[7 - i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) |
               ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}

// canonical decode: false if the value is >= r (BLSFieldElement rule)
M3X_FR_FN bool fr_from_be32(fr &r, const uint8_t *b) {
  uint32_t s[8];
  fr_limbs_from_be32(s, b);
  if (fr_ge_r(s)) return false;
  fr_from_std(r, s);
  return true;
}

// hash_to_bls_field: a 256-bit big-endian value reduced mod r
// (2^256 < 3r, so at most two subtractions)
M3X_FR_FN void fr_from_be32_reduce(fr &r, const uint8_t *b) {
  uint32_t s[8];
  fr_limbs_from_be32(s, b);
  if (fr_ge_r(s)) fr_sub_r(s);
  if (fr_ge_r(s)) fr_sub_r(s);
  fr_from_std(r, s);
}

M3X_FR_FN void fr_to_be32(const fr &a, uint8_t *b) {
  uint32_t s[8];
  fr_to_std(s, a);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    b[4 * i] = (uint8_t)(s[7 - i] >> 24);
    b[4 * i + 1] = (uint8_t)(s[7 - i] >> 16);
    b[4 * i + 2] = (uint8_t)(s[7 - i] >> 8);
    b[4 * i + 3] = (uint8_t)s[7 - i];
  }
}

// MSB-first pow by a little-endian 32-bit limb exponent; a^0 = 1
M3X_FR_FN void fr_pow(fr &r, const fr &a, const uint32_t *e, int n) {
  fr acc;
  fr_one(acc);
  bool started = false;
  for (int i = n - 1; i >= 0; i--) {
    for (int b = 31; b >= 0; b--) {
      if (started) fr_sqr(acc, acc);
      if ((e[i] >> b) & 1) {
        if (started)
          fr_mul(acc, acc, a);
        else {
          acc = a;
          started = true;
        }
      }
    }
  }
  r = acc;
}

// Fermat inverse a^(r-2); inv(0) = 0
M3X_FR_FN void fr_inv(fr &r, const fr &a) {
  // r - 2: FR_MOD[0] = 1 borrows from limb 1 (0xffffffff -> 0xfffffffe)
  uint32_t e[8] = {0xffffffffu, FR_MOD[1] - 1, FR_MOD[2], FR_MOD[3],
                   FR_MOD[4],   FR_MOD[5],     FR_MOD[6], FR_MOD[7]};
  fr_pow(r, a, e, 8);
}

} // namespace m3xf
