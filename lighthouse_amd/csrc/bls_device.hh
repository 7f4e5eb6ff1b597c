// BLS12-381 device arithmetic for gfx950 (hot path #1).
//
// Design (DESIGN.md §BLS batch verify): one signature set per lane, 381-bit
// Montgomery Fp on 64-bit integer MAD chains (__int128 lowers to
// v_mad_u64_u32), inversion-free Jacobian Miller loop with sparse lines
// (formulas validated against the Python reference in gen_bls_fixtures.py:
// jacobian-sparse == generic, hard-part identity, psi subgroup check — all
// asserted in-session and re-pinned by tests/golden fixtures), final
// exponentiation via the (x-1)^2(x+p)(x^2+p^2-1)+3 chain (cubed exponent —
// equivalent for the ==1 test since gcd(3, r) = 1).
//
// Fp12 values are deliberately kept in thread-local MEMORY (runtime-indexed
// arrays -> scratch): the ~130k-cycle VALU cost of an Fp12 multiply dwarfs
// the ~1KB of scratch traffic, and keeping f out of registers avoids
// catastrophic spilling in the Miller loop.
//
// Constants come from bls_consts.h (generated + numerically validated by
// tests/golden/gen_bls_fixtures.py; constexpr so device code folds them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bls_consts.h"
#include "bls_h2c_consts.h"
#include "sha256.hh"

namespace m3xb {

struct fp {
  uint64_t v[6];
}; // Montgomery form

struct fp2 {
  fp c0, c1;
};

struct g1a {
  fp x, y;
  int inf;
};
struct g1j {
  fp x, y, z;
}; // z==0 => infinity
struct g2a {
  fp2 x, y;
  int inf;
};
struct g2j {
  fp2 x, y, z;
};

// ------------------------------------------------------------------- Fp ---

__device__ __forceinline__ bool fp_ge_p(const uint64_t t[6]) {
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    if (t[i] > BLS_P[i]) return true;
    if (t[i] < BLS_P[i]) return false;
  }
  return true;
}

__device__ __forceinline__ void fp_sub_p(uint64_t t[6]) {
  unsigned __int128 bw = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    unsigned __int128 x = (unsigned __int128)t[i] - BLS_P[i] - (uint64_t)bw;
    t[i] = (uint64_t)x;
    bw = (x >> 64) & 1;
  }
}

__device__ __forceinline__ void fp_add(fp &r, const fp &a, const fp &b) {
  unsigned __int128 c = 0;
  uint64_t t[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    c += (unsigned __int128)a.v[i] + b.v[i];
    t[i] = (uint64_t)c;
    c >>= 64;
  }
  if (c || fp_ge_p(t)) fp_sub_p(t);
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = t[i];
}

__device__ __forceinline__ void fp_sub(fp &r, const fp &a, const fp &b) {
  unsigned __int128 bw = 0;
  uint64_t t[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    unsigned __int128 x = (unsigned __int128)a.v[i] - b.v[i] - (uint64_t)bw;
    t[i] = (uint64_t)x;
    bw = (x >> 64) & 1;
  }
  if (bw) {
    unsigned __int128 c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      c += (unsigned __int128)t[i] + BLS_P[i];
      t[i] = (uint64_t)c;
      c >>= 64;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = t[i];
}

__device__ __forceinline__ void fp_zero(fp &r) {
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = 0;
}

__device__ __forceinline__ void fp_neg(fp &r, const fp &a) {
  fp z;
  fp_zero(z);
  fp_sub(r, z, a);
}

__device__ __forceinline__ bool fp_is_zero(const fp &a) {
  uint64_t o = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) o |= a.v[i];
  return o == 0;
}

__device__ __forceinline__ bool fp_eq(const fp &a, const fp &b) {
  uint64_t o = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}

// Montgomery multiply, 12x32-bit limb CIOS: each inner mac is one
// v_mad_u64_u32 (32x32+64) + a 32-bit carry fold — measured 1.49x the
// 6x64-limb __int128 CIOS on gfx950 (tools/fpbench.hip, 5451 vs 8136
// cyc/mul dependent chain; dual-interleaved forms showed both are
// issue-bound). Validated bit-exact vs the 64-bit CIOS on 500k random +
// edge inputs (CPU) and on-chain on GPU. The LE u64 limb layout aliases
// to LE u32 limbs for free.
__device__ __forceinline__ void fp_mul(fp &r, const fp &a, const fp &b) {
  const uint32_t *A = reinterpret_cast<const uint32_t *>(a.v);
  const uint32_t *B = reinterpret_cast<const uint32_t *>(b.v);
  uint32_t P32[12];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    P32[2 * i] = (uint32_t)BLS_P[i];
    P32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
  }
  const uint32_t N0_32 = (uint32_t)BLS_N0; /* -p^-1 mod 2^32 */
  uint32_t t[14];
#pragma unroll
  for (int i = 0; i < 14; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) {
      uint64_t s = (uint64_t)A[j] * B[i] + t[j] + (uint32_t)c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    uint64_t s = (uint64_t)t[12] + c;
    t[12] = (uint32_t)s;
    t[13] = (uint32_t)(s >> 32);
    uint32_t m = t[0] * N0_32;
    c = ((uint64_t)m * P32[0] + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 12; j++) {
      uint64_t s2 = (uint64_t)m * P32[j] + t[j] + (uint32_t)c;
      t[j - 1] = (uint32_t)s2;
      c = s2 >> 32;
    }
    s = (uint64_t)t[12] + c;
    t[11] = (uint32_t)s;
    t[12] = t[13] + (uint32_t)(s >> 32);
    t[13] = 0;
  }
  uint64_t res[6];
#pragma unroll
  for (int i = 0; i < 6; i++)
    res[i] = (uint64_t)t[2 * i] | ((uint64_t)t[2 * i + 1] << 32);
  if (t[12] || fp_ge_p(res)) fp_sub_p(res);
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = res[i];
}

// specialized 12x32 SOS squaring: 66 cross + 12 diagonal MACs + the same
// 144-MAC Montgomery reduction = 222 MACs vs fp_mul's 288. Measured 12%
// faster on a dependent chain (tools/fpbench variant H, bit-exact) —
// pays in the 381-bit pow chains (sqrt/inv) where squarings dominate.
__device__ __forceinline__ void fp_sqr(fp &r, const fp &a) {
  const uint32_t *A = reinterpret_cast<const uint32_t *>(a.v);
  uint32_t P32[12];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    P32[2 * i] = (uint32_t)BLS_P[i];
    P32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
  }
  const uint32_t N0_32 = (uint32_t)BLS_N0;
  uint32_t t[25];
#pragma unroll
  for (int i = 0; i < 25; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 11; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = i + 1; j < 12; j++) {
      uint64_t p = (uint64_t)A[i] * A[j] + t[i + j] + (uint32_t)c;
      t[i + j] = (uint32_t)p;
      c = p >> 32;
    }
    t[i + 12] = (uint32_t)c;
  }
  uint32_t cc = 0;
#pragma unroll
  for (int i = 0; i < 24; i++) {
    uint32_t nv = (t[i] << 1) | cc;
    cc = t[i] >> 31;
    t[i] = nv;
  }
  {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
      uint64_t p = (uint64_t)A[i] * A[i] + t[2 * i] + (uint32_t)c;
      t[2 * i] = (uint32_t)p;
      uint64_t p2 = (uint64_t)t[2 * i + 1] + (p >> 32);
      t[2 * i + 1] = (uint32_t)p2;
      c = p2 >> 32;
    }
  }
  // Montgomery reduce the 24-limb square (< p^2 < p*2^384)
  uint32_t w[12];
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = t[i];
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint32_t m = w[0] * N0_32;
    uint64_t c = ((uint64_t)m * P32[0] + w[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 12; j++) {
      uint64_t p = (uint64_t)m * P32[j] + w[j] + (uint32_t)c;
      w[j - 1] = (uint32_t)p;
      c = p >> 32;
    }
    uint64_t p = (uint64_t)t[12 + i] + c + carry;
    w[11] = (uint32_t)p;
    carry = (uint32_t)(p >> 32);
  }
  uint64_t res[6];
#pragma unroll
  for (int i = 0; i < 6; i++)
    res[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  if (carry || fp_ge_p(res)) fp_sub_p(res);
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = res[i];
}

__device__ __forceinline__ void fp_one(fp &r) {
  // R mod p = mont(1): computed as R2 * 1 via montmul(1_std, R2)
  fp one_std, r2;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    one_std.v[i] = (i == 0) ? 1ull : 0ull;
    r2.v[i] = BLS_R2[i];
  }
  fp_mul(r, one_std, r2);
}

__device__ __forceinline__ void fp_from_std(fp &r, const uint64_t std[6]) {
  fp s, r2;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    s.v[i] = std[i];
    r2.v[i] = BLS_R2[i];
  }
  fp_mul(r, s, r2);
}

// compile-time-constant loads (constexpr array -> immediate limbs)
#define FP_LOAD_C(dst, NAME)                                                   \
  do {                                                                         \
    uint64_t _std[6] = {NAME[0], NAME[1], NAME[2], NAME[3], NAME[4], NAME[5]}; \
    fp_from_std(dst, _std);                                                    \
  } while (0)

__device__ __forceinline__ void fp_to_std(uint64_t std[6], const fp &a) {
  fp one_std;
#pragma unroll
  for (int i = 0; i < 6; i++) one_std.v[i] = (i == 0) ? 1ull : 0ull;
  fp t;
  fp_mul(t, a, one_std);
#pragma unroll
  for (int i = 0; i < 6; i++) std[i] = t.v[i];
}

// MSB-first pow by a little-endian limb exponent (top limb index n-1)
__device__ inline void fp_pow_limbs(fp &r, const fp &a, const uint64_t *e,
                                    int n) {
  fp acc;
  fp_one(acc);
  bool started = false;
  for (int i = n - 1; i >= 0; i--) {
    for (int b = 63; b >= 0; b--) {
      if (started) fp_sqr(acc, acc);
      if ((e[i] >> b) & 1) {
        if (started)
          fp_mul(acc, acc, a);
        else {
          acc = a;
          started = true;
        }
      }
    }
  }
  r = acc;
}

__device__ inline void fp_inv(fp &r, const fp &a) {
  uint64_t e[6] = {BLS_P[0] - 2, BLS_P[1], BLS_P[2],
                   BLS_P[3], BLS_P[4], BLS_P[5]};
  fp_pow_limbs(r, a, e, 6);
}

__device__ __forceinline__ void fp_sel(fp &r, bool c, const fp &a,
                                       const fp &b) {
#pragma unroll
  for (int i = 0; i < 6; i++) r.v[i] = c ? a.v[i] : b.v[i];
}

// a^((p-3)/4) and a^((p+1)/4)
__device__ inline void fp_pow_m3(fp &r, const fp &a) {
  // (p-3)/4: p[0] = ...aaab so p-3 borrows nothing
  uint64_t t[6] = {BLS_P[0] - 3, BLS_P[1], BLS_P[2],
                   BLS_P[3], BLS_P[4], BLS_P[5]};
  uint64_t e[6];
#pragma unroll
  for (int i = 0; i < 6; i++)
    e[i] = (t[i] >> 2) | (i < 5 ? (t[i + 1] << 62) : 0);
  fp_pow_limbs(r, a, e, 6);
}
__device__ inline void fp_pow_p1(fp &r, const fp &a) {
  // (p+1)/4: p+1 has no carry past limb 0
  uint64_t t[6] = {BLS_P[0] + 1, BLS_P[1], BLS_P[2],
                   BLS_P[3], BLS_P[4], BLS_P[5]};
  uint64_t e[6];
#pragma unroll
  for (int i = 0; i < 6; i++)
    e[i] = (t[i] >> 2) | (i < 5 ? (t[i + 1] << 62) : 0);
  fp_pow_limbs(r, a, e, 6);
}

// sqrt candidate a^((p+1)/4); returns false if a is not a square
__device__ inline bool fp_sqrt(fp &r, const fp &a) {
  fp s, s2;
  fp_pow_p1(s, a);
  fp_sqr(s2, s);
  if (!fp_eq(s2, a)) return false;
  r = s;
  return true;
}

// sqrt AND inverse-sqrt in ONE pow (p = 3 mod 4): u = a^((p-3)/4) is
// 1/sqrt(a) for square a (u*s = a^((p-1)/2) = 1), s = u*a = a^((p+1)/4).
// Lets callers replace a sqrt-then-invert pair (two 381-bit pows) with
// one pow + one mul. Returns false for non-squares (s, u then invalid).
__device__ inline bool fp_sqrt_ui(fp &s, fp &u, const fp &a) {
  fp_pow_m3(u, a);
  fp_mul(s, u, a);
  fp s2;
  fp_sqr(s2, s);
  return fp_eq(s2, a);
}

// standard-form compare against (p-1)/2 ("lexicographically largest")
__device__ inline bool fp_gt_half(const fp &a) {
  uint64_t s[6];
  fp_to_std(s, a);
  uint64_t pm1[6] = {BLS_P[0] - 1, BLS_P[1], BLS_P[2],
                     BLS_P[3], BLS_P[4], BLS_P[5]};
  uint64_t h[6];
#pragma unroll
  for (int i = 0; i < 6; i++)
    h[i] = (pm1[i] >> 1) | (i < 5 ? (pm1[i + 1] << 63) : 0);
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    if (s[i] > h[i]) return true;
    if (s[i] < h[i]) return false;
  }
  return false;
}

__device__ inline bool fp_is_odd_std(const fp &a) {
  uint64_t s[6];
  fp_to_std(s, a);
  return s[0] & 1;
}

// 48-byte big-endian -> fp (Montgomery); returns false if >= p
__device__ inline bool fp_from_be48(fp &r, const uint8_t *b) {
  uint64_t s[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w = (w << 8) | b[8 * i + j];
    s[5 - i] = w;
  }
  if (fp_ge_p(s)) return false;
  fp_from_std(r, s);
  return true;
}

__device__ inline void fp_to_be48(const fp &a, uint8_t *b) {
  uint64_t s[6];
  fp_to_std(s, a);
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 8; j++)
      b[8 * i + j] = (uint8_t)(s[5 - i] >> (56 - 8 * j));
}

// ------------------------------------------------------------------ Fp2 ---

__device__ __forceinline__ void fp2_add(fp2 &r, const fp2 &a, const fp2 &b) {
  fp_add(r.c0, a.c0, b.c0);
  fp_add(r.c1, a.c1, b.c1);
}
__device__ __forceinline__ void fp2_sub(fp2 &r, const fp2 &a, const fp2 &b) {
  fp_sub(r.c0, a.c0, b.c0);
  fp_sub(r.c1, a.c1, b.c1);
}
__device__ __forceinline__ void fp2_neg(fp2 &r, const fp2 &a) {
  fp_neg(r.c0, a.c0);
  fp_neg(r.c1, a.c1);
}
__device__ __forceinline__ void fp2_dbl(fp2 &r, const fp2 &a) {
  fp2_add(r, a, a);
}
__device__ __forceinline__ void fp2_zero(fp2 &r) {
  fp_zero(r.c0);
  fp_zero(r.c1);
}
__device__ __forceinline__ void fp2_one(fp2 &r) {
  fp_one(r.c0);
  fp_zero(r.c1);
}
__device__ __forceinline__ void fp2_conj(fp2 &r, const fp2 &a) {
  r.c0 = a.c0;
  fp_neg(r.c1, a.c1);
}
__device__ __forceinline__ bool fp2_is_zero(const fp2 &a) {
  return fp_is_zero(a.c0) && fp_is_zero(a.c1);
}
__device__ __forceinline__ bool fp2_eq(const fp2 &a, const fp2 &b) {
  return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1);
}

__device__ __forceinline__ void fp2_mul(fp2 &r, const fp2 &a, const fp2 &b) {
  fp t0, t1, s0, s1, m;
  fp_mul(t0, a.c0, b.c0);
  fp_mul(t1, a.c1, b.c1);
  fp_add(s0, a.c0, a.c1);
  fp_add(s1, b.c0, b.c1);
  fp_mul(m, s0, s1);
  fp_sub(m, m, t0);
  fp_sub(m, m, t1);
  fp_sub(r.c0, t0, t1);
  r.c1 = m;
}

__device__ __forceinline__ void fp2_sqr(fp2 &r, const fp2 &a) {
  fp s, d, m;
  fp_add(s, a.c0, a.c1);
  fp_sub(d, a.c0, a.c1);
  fp_mul(m, a.c0, a.c1);
  fp_mul(s, s, d);
  fp_add(r.c1, m, m);
  r.c0 = s;
}

__device__ __forceinline__ void fp2_mul_fp(fp2 &r, const fp2 &a, const fp &k) {
  fp_mul(r.c0, a.c0, k);
  fp_mul(r.c1, a.c1, k);
}

// small-integer multiply (for 2x/3x/8x)
__device__ __forceinline__ void fp2_mul_small(fp2 &r, const fp2 &a, int k) {
  fp2 acc = a;
  for (int i = 1; i < k; i++) fp2_add(acc, acc, a);
  r = acc;
}

__device__ inline void fp2_inv(fp2 &r, const fp2 &a) {
  fp n, t0, t1;
  fp_sqr(t0, a.c0);
  fp_sqr(t1, a.c1);
  fp_add(n, t0, t1);
  fp_inv(n, n);
  fp_mul(r.c0, a.c0, n);
  fp_mul(t0, a.c1, n);
  fp_neg(r.c1, t0);
}

// multiply by xi = 1+u: (c0 - c1) + (c0 + c1) u
__device__ __forceinline__ void fp2_mul_xi(fp2 &r, const fp2 &a) {
  fp t0, t1;
  fp_sub(t0, a.c0, a.c1);
  fp_add(t1, a.c0, a.c1);
  r.c0 = t0;
  r.c1 = t1;
}

__device__ __forceinline__ void fp2_sel(fp2 &r, bool c, const fp2 &a,
                                        const fp2 &b) {
  fp_sel(r.c0, c, a.c0, b.c0);
  fp_sel(r.c1, c, a.c1, b.c1);
}

__device__ __forceinline__ void fp2_norm(fp &n, const fp2 &a) {
  fp t;
  fp_sqr(n, a.c0);
  fp_sqr(t, a.c1);
  fp_add(n, n, t);
}

// A root of a = a0 + a1 i (a1 != 0) given s with s^2 = N(a): ONE pow and a
// select, no retry. d = (a0+s)/2, u = d^((p-3)/4), t = u d, so t^2 = +-d.
// "+": (t, a1 u/2), the textbook form (u = 1/t). "-": d is a non-residue,
// u t = d^((p-1)/2) = -1 gives 1/t = -u, and (a0+s)(a0-s)/4 = -a1^2/4 makes
// (-a1 u/2, t) the root that the retry on (a0-s)/2 used to find.
// Meaningless (not a root) when s^2 != N(a): callers check or know.
__device__ inline void fp2_sqrt_from_norm_root(fp2 &r, const fp2 &a,
                                               const fp &s) {
  fp inv2, d, u, t, h, nh, t2;
  FP_LOAD_C(inv2, FP_TWO_INV); // constant 2^-1 (generator-emitted)
  fp_add(d, a.c0, s);
  fp_mul(d, d, inv2);
  fp_pow_m3(u, d);
  fp_mul(t, u, d);
  fp_mul(h, a.c1, u);
  fp_mul(h, h, inv2);
  fp_neg(nh, h);
  fp_sqr(t2, t);
  bool plus = fp_eq(t2, d);
  fp_sel(r.c0, plus, t, nh);
  fp_sel(r.c1, plus, h, t);
}

__device__ inline bool fp2_sqrt(fp2 &r, const fp2 &a) {
  if (fp2_is_zero(a)) {
    fp2_zero(r);
    return true;
  }
  if (fp_is_zero(a.c1)) { // rare: the generic path has d = 0 here
    fp s;
    if (fp_sqrt(s, a.c0)) {
      r.c0 = s;
      fp_zero(r.c1);
      return true;
    }
    fp na;
    fp_neg(na, a.c0);
    if (!fp_sqrt(s, na)) return false;
    fp_zero(r.c0);
    r.c1 = s;
    return true;
  }
  fp n, s;
  fp2_norm(n, a);
  if (!fp_sqrt(s, n)) return false;
  fp2 cand, sq;
  fp2_sqrt_from_norm_root(cand, a, s);
  fp2_sqr(sq, cand);
  if (!fp2_eq(sq, a)) return false;
  r = cand;
  return true;
}

__device__ inline bool fp2_gt_half_lex(const fp2 &y) {
  if (!fp_is_zero(y.c1)) return fp_gt_half(y.c1);
  if (!fp_is_zero(y.c0)) return fp_gt_half(y.c0);
  return false;
}

__device__ inline int fp2_sgn0(const fp2 &x) {
  int s0 = fp_is_odd_std(x.c0) ? 1 : 0;
  int z0 = fp_is_zero(x.c0) ? 1 : 0;
  int s1 = fp_is_odd_std(x.c1) ? 1 : 0;
  return s0 | (z0 & s1);
}

#define FP2_LOAD_C(dst, NAME)                                                  \
  do {                                                                         \
    FP_LOAD_C((dst).c0, NAME##_C0);                                            \
    FP_LOAD_C((dst).c1, NAME##_C1);                                            \
  } while (0)

// ------------------------------------------------------------- G1 points ---

__device__ __forceinline__ bool g1j_is_inf(const g1j &p) {
  return fp_is_zero(p.z);
}

__device__ __forceinline__ void g1j_set_inf(g1j &p) {
  fp_zero(p.x);
  fp_zero(p.y);
  fp_zero(p.z);
}

__device__ inline void g1j_from_aff(g1j &r, const g1a &a) {
  if (a.inf) {
    g1j_set_inf(r);
    return;
  }
  r.x = a.x;
  r.y = a.y;
  fp_one(r.z);
}

__device__ inline void g1j_to_aff(g1a &r, const g1j &p) {
  if (g1j_is_inf(p)) {
    r.inf = 1;
    fp_zero(r.x);
    fp_zero(r.y);
    return;
  }
  fp zi, zi2, zi3;
  fp_inv(zi, p.z);
  fp_sqr(zi2, zi);
  fp_mul(zi3, zi2, zi);
  fp_mul(r.x, p.x, zi2);
  fp_mul(r.y, p.y, zi3);
  r.inf = 0;
}

__device__ inline void g1j_dbl(g1j &r, const g1j &p) {
  if (g1j_is_inf(p)) {
    r = p;
    return;
  }
  fp A, B, C, D, E, F, t;
  fp_sqr(A, p.x);
  fp_sqr(B, p.y);
  fp_sqr(C, B);
  fp_add(D, p.x, B);
  fp_sqr(D, D);
  fp_sub(D, D, A);
  fp_sub(D, D, C);
  fp_add(D, D, D);
  fp_add(E, A, A);
  fp_add(E, E, A);
  fp_sqr(F, E);
  fp_sub(F, F, D);
  fp_sub(F, F, D);
  fp_mul(t, p.y, p.z);
  fp_add(r.z, t, t);
  fp_sub(t, D, F);
  fp_mul(t, E, t);
  fp_add(C, C, C);
  fp_add(C, C, C);
  fp_add(C, C, C);
  fp_sub(r.y, t, C);
  r.x = F;
}

__device__ inline void g1j_add(g1j &r, const g1j &p, const g1j &q) {
  if (g1j_is_inf(p)) {
    r = q;
    return;
  }
  if (g1j_is_inf(q)) {
    r = p;
    return;
  }
  fp z1z1, z2z2, u1, u2, s1, s2, t;
  fp_sqr(z1z1, p.z);
  fp_sqr(z2z2, q.z);
  fp_mul(u1, p.x, z2z2);
  fp_mul(u2, q.x, z1z1);
  fp_mul(t, q.z, z2z2);
  fp_mul(s1, p.y, t);
  fp_mul(t, p.z, z1z1);
  fp_mul(s2, q.y, t);
  if (fp_eq(u1, u2)) {
    if (fp_eq(s1, s2)) {
      g1j_dbl(r, p);
      return;
    }
    g1j_set_inf(r);
    return;
  }
  fp h, i, j, rr, v, y3, z3;
  fp_sub(h, u2, u1);
  fp_add(i, h, h);
  fp_sqr(i, i);
  fp_mul(j, h, i);
  fp_sub(rr, s2, s1);
  fp_add(rr, rr, rr);
  fp_mul(v, u1, i);
  fp_sqr(t, rr);
  fp_sub(t, t, j);
  fp_sub(t, t, v);
  fp_sub(t, t, v);
  fp_sub(y3, v, t);
  fp_mul(y3, rr, y3);
  fp s1j;
  fp_mul(s1j, s1, j);
  fp_add(s1j, s1j, s1j);
  fp_sub(y3, y3, s1j);
  fp_add(z3, p.z, q.z);
  fp_sqr(z3, z3);
  fp_sub(z3, z3, z1z1);
  fp_sub(z3, z3, z2z2);
  fp_mul(z3, z3, h);
  r.x = t;
  r.y = y3;
  r.z = z3;
}

// mixed add (Jacobian += affine, madd-2007-bl: 7M+4S vs 11M+5S general)
__device__ inline void g1j_add_aff(g1j &r, const g1j &p, const g1a &q) {
  if (q.inf) {
    r = p;
    return;
  }
  if (g1j_is_inf(p)) {
    g1j_from_aff(r, q);
    return;
  }
  fp z1z1, u2, s2, t;
  fp_sqr(z1z1, p.z);
  fp_mul(u2, q.x, z1z1);
  fp_mul(t, p.z, z1z1);
  fp_mul(s2, q.y, t);
  if (fp_eq(u2, p.x)) {
    if (fp_eq(s2, p.y)) {
      g1j_dbl(r, p);
      return;
    }
    g1j_set_inf(r);
    return;
  }
  fp h, hh, i, j, rr, v, x3, y3, z3;
  fp_sub(h, u2, p.x);
  fp_sqr(hh, h);
  fp_add(i, hh, hh);
  fp_add(i, i, i); // 4*HH
  fp_mul(j, h, i);
  fp_sub(rr, s2, p.y);
  fp_add(rr, rr, rr);
  fp_mul(v, p.x, i);
  fp_sqr(x3, rr);
  fp_sub(x3, x3, j);
  fp_sub(x3, x3, v);
  fp_sub(x3, x3, v);
  fp_sub(y3, v, x3);
  fp_mul(y3, rr, y3);
  fp_mul(t, p.y, j);
  fp_add(t, t, t);
  fp_sub(y3, y3, t);
  fp_add(z3, p.z, h);
  fp_sqr(z3, z3);
  fp_sub(z3, z3, z1z1);
  fp_sub(z3, z3, hh);
  r.x = x3;
  r.y = y3;
  r.z = z3;
}

// [k]P with a Jacobian base (full adds; used where the base is already
// Jacobian, e.g. the wave-aggregated pubkey sum)
__device__ inline void g1j_mul_be_j(g1j &r, const g1j &base,
                                    const uint8_t *be, int nbytes) {
  g1j acc;
  g1j_set_inf(acc);
  for (int i = 0; i < nbytes; i++) {
    uint8_t byte = be[i];
    for (int b = 7; b >= 0; b--) {
      g1j_dbl(acc, acc);
      if ((byte >> b) & 1) g1j_add(acc, acc, base);
    }
  }
  r = acc;
}

__device__ inline void g1j_mul_be(g1j &r, const g1a &p, const uint8_t *be,
                                  int nbytes) {
  g1j acc, base;
  g1j_set_inf(acc);
  g1j_from_aff(base, p);
  for (int i = 0; i < nbytes; i++) {
    uint8_t byte = be[i];
    for (int b = 7; b >= 0; b--) {
      g1j_dbl(acc, acc);
      if ((byte >> b) & 1) g1j_add(acc, acc, base);
    }
  }
  r = acc;
}

// ------------------------------------------------------------- G2 points ---

__device__ __forceinline__ bool g2j_is_inf(const g2j &p) {
  return fp2_is_zero(p.z);
}

__device__ __forceinline__ void g2j_set_inf(g2j &p) {
  fp2_zero(p.x);
  fp2_zero(p.y);
  fp2_zero(p.z);
}

__device__ inline void g2j_from_aff(g2j &r, const g2a &a) {
  if (a.inf) {
    g2j_set_inf(r);
    return;
  }
  r.x = a.x;
  r.y = a.y;
  fp2_one(r.z);
}

__device__ inline void g2j_to_aff(g2a &r, const g2j &p) {
  if (g2j_is_inf(p)) {
    r.inf = 1;
    fp2_zero(r.x);
    fp2_zero(r.y);
    return;
  }
  fp2 zi, zi2, zi3;
  fp2_inv(zi, p.z);
  fp2_sqr(zi2, zi);
  fp2_mul(zi3, zi2, zi);
  fp2_mul(r.x, p.x, zi2);
  fp2_mul(r.y, p.y, zi3);
  r.inf = 0;
}

__device__ inline void g2j_dbl(g2j &r, const g2j &p) {
  if (g2j_is_inf(p)) {
    r = p;
    return;
  }
  fp2 A, B, C, D, E, F, t;
  fp2_sqr(A, p.x);
  fp2_sqr(B, p.y);
  fp2_sqr(C, B);
  fp2_add(D, p.x, B);
  fp2_sqr(D, D);
  fp2_sub(D, D, A);
  fp2_sub(D, D, C);
  fp2_dbl(D, D);
  fp2_dbl(E, A);
  fp2_add(E, E, A);
  fp2_sqr(F, E);
  fp2_sub(F, F, D);
  fp2_sub(F, F, D);
  fp2_mul(t, p.y, p.z);
  fp2_dbl(r.z, t);
  fp2_sub(t, D, F);
  fp2_mul(t, E, t);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_sub(r.y, t, C);
  r.x = F;
}

__device__ inline void g2j_add(g2j &r, const g2j &p, const g2j &q) {
  if (g2j_is_inf(p)) {
    r = q;
    return;
  }
  if (g2j_is_inf(q)) {
    r = p;
    return;
  }
  fp2 z1z1, z2z2, u1, u2, s1, s2, t;
  fp2_sqr(z1z1, p.z);
  fp2_sqr(z2z2, q.z);
  fp2_mul(u1, p.x, z2z2);
  fp2_mul(u2, q.x, z1z1);
  fp2_mul(t, q.z, z2z2);
  fp2_mul(s1, p.y, t);
  fp2_mul(t, p.z, z1z1);
  fp2_mul(s2, q.y, t);
  if (fp2_eq(u1, u2)) {
    if (fp2_eq(s1, s2)) {
      g2j_dbl(r, p);
      return;
    }
    g2j_set_inf(r);
    return;
  }
  fp2 h, i, j, rr, v, y3, z3, s1j;
  fp2_sub(h, u2, u1);
  fp2_dbl(i, h);
  fp2_sqr(i, i);
  fp2_mul(j, h, i);
  fp2_sub(rr, s2, s1);
  fp2_dbl(rr, rr);
  fp2_mul(v, u1, i);
  fp2_sqr(t, rr);
  fp2_sub(t, t, j);
  fp2_sub(t, t, v);
  fp2_sub(t, t, v);
  fp2_sub(y3, v, t);
  fp2_mul(y3, rr, y3);
  fp2_mul(s1j, s1, j);
  fp2_dbl(s1j, s1j);
  fp2_sub(y3, y3, s1j);
  fp2_add(z3, p.z, q.z);
  fp2_sqr(z3, z3);
  fp2_sub(z3, z3, z1z1);
  fp2_sub(z3, z3, z2z2);
  fp2_mul(z3, z3, h);
  r.x = t;
  r.y = y3;
  r.z = z3;
}

// mixed add (Jacobian += affine), the G2 mirror of g1j_add_aff
__device__ inline void g2j_add_aff(g2j &r, const g2j &p, const g2a &q) {
  if (q.inf) {
    r = p;
    return;
  }
  if (g2j_is_inf(p)) {
    g2j_from_aff(r, q);
    return;
  }
  fp2 z1z1, u2, s2, t;
  fp2_sqr(z1z1, p.z);
  fp2_mul(u2, q.x, z1z1);
  fp2_mul(t, p.z, z1z1);
  fp2_mul(s2, q.y, t);
  if (fp2_eq(u2, p.x)) {
    if (fp2_eq(s2, p.y)) {
      g2j_dbl(r, p);
      return;
    }
    g2j_set_inf(r);
    return;
  }
  fp2 h, hh, i, j, rr, v, x3, y3, z3;
  fp2_sub(h, u2, p.x);
  fp2_sqr(hh, h);
  fp2_dbl(i, hh);
  fp2_dbl(i, i);
  fp2_mul(j, h, i);
  fp2_sub(rr, s2, p.y);
  fp2_dbl(rr, rr);
  fp2_mul(v, p.x, i);
  fp2_sqr(x3, rr);
  fp2_sub(x3, x3, j);
  fp2_sub(x3, x3, v);
  fp2_sub(x3, x3, v);
  fp2_sub(y3, v, x3);
  fp2_mul(y3, rr, y3);
  fp2_mul(t, p.y, j);
  fp2_dbl(t, t);
  fp2_sub(y3, y3, t);
  fp2_add(z3, p.z, h);
  fp2_sqr(z3, z3);
  fp2_sub(z3, z3, z1z1);
  fp2_sub(z3, z3, hh);
  r.x = x3;
  r.y = y3;
  r.z = z3;
}

// a stored sig_aff entry (z = 1: affine x, y; z = 0: infinity) as a g2a
__device__ __forceinline__ void sig_aff_load(g2a &sig, const g2j &sj) {
  sig.x = sj.x;
  sig.y = sj.y;
  sig.inf = g2j_is_inf(sj) ? 1 : 0;
}

// [k1]P and [k2]P with ONE shared doubling chain of the base (LSB-first
// double-and-add) — the subgroup-check [|x|]sigma and the batch [r]sigma
// share sigma's doublings.
__device__ inline void g2j_mul2_u64(g2j &r1, g2j &r2, const g2a &p,
                                    uint64_t k1, uint64_t k2) {
  g2j base, a1, a2;
  g2j_from_aff(base, p);
  g2j_set_inf(a1);
  a2 = a1;
  for (int b = 0; b < 64; b++) {
    if ((k1 >> b) & 1) g2j_add(a1, a1, base);
    if ((k2 >> b) & 1) g2j_add(a2, a2, base);
    if (b < 63 && ((k1 | k2) >> (b + 1)) != 0) g2j_dbl(base, base);
  }
  r1 = a1;
  r2 = a2;
}

__device__ inline void g2j_mul_be(g2j &r, const g2a &p, const uint8_t *be,
                                  int nbytes) {
  g2j acc, base;
  g2j_set_inf(acc);
  g2j_from_aff(base, p);
  for (int i = 0; i < nbytes; i++) {
    uint8_t byte = be[i];
    for (int b = 7; b >= 0; b--) {
      g2j_dbl(acc, acc);
      if ((byte >> b) & 1) g2j_add(acc, acc, base);
    }
  }
  r = acc;
}

__device__ inline void g2j_mul_u64(g2j &r, const g2a &p, uint64_t k) {
  uint8_t be[8];
#pragma unroll
  for (int i = 0; i < 8; i++) be[i] = (uint8_t)(k >> (56 - 8 * i));
  g2j_mul_be(r, p, be, 8);
}

__device__ inline void g2_b2(fp2 &b2) {
  fp one, four;
  fp_one(one);
  fp_add(four, one, one);
  fp_add(four, four, four);
  fp2 f;
  f.c0 = four;
  fp_zero(f.c1);
  fp2_mul_xi(b2, f);
}

// psi endomorphism (constants validated by the generator)
__device__ inline void psi_g2(g2a &r, const g2a &p) {
  if (p.inf) {
    r = p;
    return;
  }
  fp2 cx, cy, t;
  FP2_LOAD_C(cx, PSI_CX);
  FP2_LOAD_C(cy, PSI_CY);
  fp2_conj(t, p.x);
  fp2_mul(r.x, t, cx);
  fp2_conj(t, p.y);
  fp2_mul(r.y, t, cy);
  r.inf = 0;
}

// the subgroup check's compare: psi(Q) == -xq for an affine, finite Q and
// xq = [|x|]Q Jacobian (x < 0), cross-multiplied so nothing is inverted
__device__ inline bool psi_eq_neg(const g2a &q, const g2j &xq) {
  if (g2j_is_inf(xq)) return false;
  g2a ps;
  psi_g2(ps, q);
  fp2 z2, z3, lx, ly, ny;
  fp2_sqr(z2, xq.z);
  fp2_mul(z3, z2, xq.z);
  fp2_mul(lx, ps.x, z2);
  fp2_neg(ny, xq.y);
  fp2_mul(ly, ps.y, z3);
  return fp2_eq(lx, xq.x) && fp2_eq(ly, ny);
}

// fast G2 subgroup check: psi(Q) == -[|x|]Q (validated vs [r]Q in Python)
__device__ inline bool g2_in_subgroup(const g2a &p) {
  if (p.inf) return true;
  g2j xq;
  g2j_mul_u64(xq, p, BLS_X_ABS);
  return psi_eq_neg(p, xq);
}

// G1 subgroup check: [r]P == O, r as 32 big-endian bytes
__device__ inline bool g1_in_subgroup(const g1a &p) {
  uint8_t be[32];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint64_t limb = BLS_ORDER[3 - i];
#pragma unroll
    for (int j = 0; j < 8; j++) be[8 * i + j] = (uint8_t)(limb >> (56 - 8 * j));
  }
  g1j t;
  g1j_mul_be(t, p, be, 32);
  return g1j_is_inf(t);
}

// ---------------------------------------------------------- serialization ---

__device__ inline int g1_decompress(g1a &r, const uint8_t *in) {
  uint8_t flags = in[0];
  if (!(flags & 0x80)) return -1;
  if (flags & 0x40) {
    if ((flags & 0x3F) != 0) return -1;
    for (int i = 1; i < 48; i++)
      if (in[i]) return -1;
    r.inf = 1;
    fp_zero(r.x);
    fp_zero(r.y);
    return 0;
  }
  uint8_t xb[48];
  for (int i = 0; i < 48; i++) xb[i] = in[i];
  xb[0] &= 0x1F;
  if (!fp_from_be48(r.x, xb)) return -1;
  fp rhs, one, b1;
  fp_sqr(rhs, r.x);
  fp_mul(rhs, rhs, r.x);
  fp_one(one);
  fp_add(b1, one, one);
  fp_add(b1, b1, b1);
  fp_add(rhs, rhs, b1);
  if (!fp_sqrt(r.y, rhs)) return -1;
  if (fp_gt_half(r.y) != ((flags & 0x20) != 0)) fp_neg(r.y, r.y);
  r.inf = 0;
  return 0;
}

// trusted variant for pubkey-cache bytes: range checks only, no on-curve
// re-verification (the cache validated once at build — the same contract
// as blst's pk_validate=false flags in verify_multiple_aggregate_signatures)
__device__ inline int g1_from_uncomp_trusted(g1a &r, const uint8_t *in) {
  if (in[0] & 0x40) {
    for (int i = 0; i < 96; i++)
      if (in[i] != (i == 0 ? 0x40 : 0)) return -1;
    r.inf = 1;
    fp_zero(r.x);
    fp_zero(r.y);
    return 0;
  }
  if (!fp_from_be48(r.x, in)) return -1;
  if (!fp_from_be48(r.y, in + 48)) return -1;
  r.inf = 0;
  return 0;
}

__device__ inline void g1_to_uncomp(const g1a &p, uint8_t *out) {
  if (p.inf) {
    for (int i = 0; i < 96; i++) out[i] = 0;
    out[0] = 0x40;
    return;
  }
  fp_to_be48(p.x, out);
  fp_to_be48(p.y, out + 48);
}

__device__ inline int g2_decompress(g2a &r, const uint8_t *in) {
  uint8_t flags = in[0];
  if (!(flags & 0x80)) return -1;
  if (flags & 0x40) {
    if ((flags & 0x3F) != 0) return -1;
    for (int i = 1; i < 96; i++)
      if (in[i]) return -1;
    r.inf = 1;
    fp2_zero(r.x);
    fp2_zero(r.y);
    return 0;
  }
  uint8_t b[48];
  for (int i = 0; i < 48; i++) b[i] = in[i];
  b[0] &= 0x1F;
  if (!fp_from_be48(r.x.c1, b)) return -1; /* wire order: c1 || c0 */
  if (!fp_from_be48(r.x.c0, in + 48)) return -1;
  fp2 rhs, b2;
  fp2_sqr(rhs, r.x);
  fp2_mul(rhs, rhs, r.x);
  g2_b2(b2);
  fp2_add(rhs, rhs, b2);
  if (!fp2_sqrt(r.y, rhs)) return -1;
  if (fp2_gt_half_lex(r.y) != ((flags & 0x20) != 0)) fp2_neg(r.y, r.y);
  r.inf = 0;
  return 0;
}

// ------------------------------------------------------------------ Fp12 ---
// Fp12 = Fp2[w]/(w^6 - xi), stored as 12 fp slots (c_k = slots 2k, 2k+1) in
// thread-local memory (runtime indexing -> scratch; see header comment).

struct fp12m {
  fp s[12];
};

__device__ inline void f12_one(fp12m &r) {
  for (int i = 0; i < 12; i++) fp_zero(r.s[i]);
  fp_one(r.s[0]);
}

__device__ inline void f12_copy(fp12m &r, const fp12m &a) {
  for (int i = 0; i < 12; i++) r.s[i] = a.s[i];
}

__device__ __forceinline__ void f12_get(const fp12m &a, int k, fp2 &c) {
  c.c0 = a.s[2 * k];
  c.c1 = a.s[2 * k + 1];
}
__device__ __forceinline__ void f12_set(fp12m &a, int k, const fp2 &c) {
  a.s[2 * k] = c.c0;
  a.s[2 * k + 1] = c.c1;
}

// Fp6 helpers over the packed fp12m layout: the tower view is
// A = (c0,c2,c4), B = (c1,c3,c5) with f = A + w*B, w^2 = v,
// Fp6 = Fp2[v]/(v^3 - xi). Index mapping validated against the schoolbook
// degree-6 multiply in Python (gen_bls_fixtures arithmetic).
struct fp6 {
  fp2 c[3];
};

__device__ __forceinline__ void f6_add(fp6 &r, const fp6 &a, const fp6 &b) {
  fp2_add(r.c[0], a.c[0], b.c[0]);
  fp2_add(r.c[1], a.c[1], b.c[1]);
  fp2_add(r.c[2], a.c[2], b.c[2]);
}
__device__ __forceinline__ void f6_sub(fp6 &r, const fp6 &a, const fp6 &b) {
  fp2_sub(r.c[0], a.c[0], b.c[0]);
  fp2_sub(r.c[1], a.c[1], b.c[1]);
  fp2_sub(r.c[2], a.c[2], b.c[2]);
}
__device__ __forceinline__ void f6_mul_v(fp6 &r, const fp6 &a) {
  fp2 t;
  fp2_mul_xi(t, a.c[2]);
  r.c[2] = a.c[1];
  r.c[1] = a.c[0];
  r.c[0] = t;
}
// Karatsuba Fp6 multiply (6 fp2 muls vs 9 schoolbook) with the v^3 = xi
// reduction folded in: v_i = a_i b_i,
//   c0 = v0 + xi((a1+a2)(b1+b2) - v1 - v2)
//   c1 = (a0+a1)(b0+b1) - v0 - v1 + xi v2
//   c2 = (a0+a2)(b0+b2) - v0 - v2 + v1
// r may alias a or b (r is written after the last read of either).
__device__ __forceinline__ void f6_mul(fp6 &r, const fp6 &a, const fp6 &b) {
  fp2 v0, v1, v2, m12, m01, m02, s, t;
  fp2_mul(v0, a.c[0], b.c[0]);
  fp2_mul(v1, a.c[1], b.c[1]);
  fp2_mul(v2, a.c[2], b.c[2]);
  fp2_add(s, a.c[1], a.c[2]);
  fp2_add(t, b.c[1], b.c[2]);
  fp2_mul(m12, s, t);
  fp2_add(s, a.c[0], a.c[1]);
  fp2_add(t, b.c[0], b.c[1]);
  fp2_mul(m01, s, t);
  fp2_add(s, a.c[0], a.c[2]);
  fp2_add(t, b.c[0], b.c[2]);
  fp2_mul(m02, s, t);
  fp2_sub(m12, m12, v1);
  fp2_sub(m12, m12, v2);
  fp2_mul_xi(m12, m12);
  fp2_add(r.c[0], v0, m12);
  fp2_sub(m01, m01, v0);
  fp2_sub(m01, m01, v1);
  fp2_mul_xi(t, v2);
  fp2_add(r.c[1], m01, t);
  fp2_sub(m02, m02, v0);
  fp2_sub(m02, m02, v2);
  fp2_add(r.c[2], m02, v1);
}

// Fp6 times the Fp2 scalar (k,0,0): 3 fp2 muls
__device__ __forceinline__ void f6_mul_fp2(fp6 &r, const fp6 &a,
                                           const fp2 &k) {
  fp2_mul(r.c[0], a.c[0], k);
  fp2_mul(r.c[1], a.c[1], k);
  fp2_mul(r.c[2], a.c[2], k);
}

// Fp6 times the two-term operand (0,b1,b2): 5 fp2 muls,
//   c0 = xi(a1b2 + a2b1), c1 = a0b1 + xi a2b2, c2 = a0b2 + a1b1
// with a1b2 + a2b1 = (a1+a2)(b1+b2) - a1b1 - a2b2. r must not alias a.
__device__ __forceinline__ void f6_mul_012s(fp6 &r, const fp6 &a,
                                            const fp2 &b1, const fp2 &b2) {
  fp2 v1, v2, s, t;
  fp2_mul(v1, a.c[1], b1);
  fp2_mul(v2, a.c[2], b2);
  fp2_add(s, a.c[1], a.c[2]);
  fp2_add(t, b1, b2);
  fp2_mul(s, s, t);
  fp2_sub(s, s, v1);
  fp2_sub(s, s, v2);
  fp2_mul_xi(r.c[0], s);
  fp2_mul(s, a.c[0], b1);
  fp2_mul_xi(t, v2);
  fp2_add(r.c[1], s, t);
  fp2_mul(s, a.c[0], b2);
  fp2_add(r.c[2], s, v1);
}

__device__ __forceinline__ void f12_split(const fp12m &f, fp6 &A, fp6 &B) {
  f12_get(f, 0, A.c[0]);
  f12_get(f, 2, A.c[1]);
  f12_get(f, 4, A.c[2]);
  f12_get(f, 1, B.c[0]);
  f12_get(f, 3, B.c[1]);
  f12_get(f, 5, B.c[2]);
}
__device__ __forceinline__ void f12_join(fp12m &f, const fp6 &A,
                                         const fp6 &B) {
  f12_set(f, 0, A.c[0]);
  f12_set(f, 2, A.c[1]);
  f12_set(f, 4, A.c[2]);
  f12_set(f, 1, B.c[0]);
  f12_set(f, 3, B.c[1]);
  f12_set(f, 5, B.c[2]);
}

// r = a * b via the quadratic-over-cubic tower (3 Karatsuba Fp6 muls = 18
// fp2 muls vs 36 schoolbook); r may alias a or b (inputs are split out
// first).
__device__ inline void f12_mul_nn(fp12m &r, const fp12m &a, const fp12m &b) {
  fp6 A1, B1, A2, B2, aa, bb, s1, s2, cross, even, t;
  f12_split(a, A1, B1);
  f12_split(b, A2, B2);
  f6_mul(aa, A1, A2);
  f6_mul(bb, B1, B2);
  f6_add(s1, A1, B1);
  f6_add(s2, A2, B2);
  f6_mul(cross, s1, s2);
  f6_sub(cross, cross, aa);
  f6_sub(cross, cross, bb); // A1B2 + A2B1
  f6_mul_v(t, bb);
  f6_add(even, aa, t); // A1A2 + v B1B2
  f12_join(r, even, cross);
}

// r = a^2: complex squaring, 2 Karatsuba Fp6 muls = 12 fp2 muls;
// alias-safe.
__device__ inline void f12_sqr_nn(fp12m &r, const fp12m &a) {
  fp6 A, B, m1, t, u, even, odd;
  f12_split(a, A, B);
  f6_mul(m1, A, B);
  f6_add(t, A, B);
  f6_mul_v(u, B);
  f6_add(u, A, u);
  f6_mul(t, t, u); // (A+B)(A+vB)
  f6_sub(t, t, m1);
  f6_mul_v(u, m1);
  f6_sub(even, t, u); // A^2 + v B^2
  f6_add(odd, m1, m1); // 2AB
  f12_join(r, even, odd);
}

// r = f * (a0 + a3 w^3 + a5 w^5), 14 fp2 muls (18 coefficient-wise). In
// the tower view the line is A_l = (a0,0,0), B_l = (0,a3,a5), so
//   f*l = (A A_l + v B B_l) + w((A+B)(A_l+B_l) - A A_l - B B_l)
// with A A_l a scalar product (3), B B_l a two-term product (5) and only
// the cross term dense (6). r may alias f (f is split out first).
__device__ inline void f12_line_nn(fp12m &r, const fp12m &f, const fp2 &a0,
                                   const fp2 &a3, const fp2 &a5) {
  fp6 A, B, aa, bb, s, l, cross, even;
  f12_split(f, A, B);
  f6_mul_fp2(aa, A, a0);
  f6_mul_012s(bb, B, a3, a5);
  f6_add(s, A, B);
  l.c[0] = a0;
  l.c[1] = a3;
  l.c[2] = a5;
  f6_mul(cross, s, l);
  f6_sub(cross, cross, aa);
  f6_sub(cross, cross, bb);
  f6_mul_v(s, bb);
  f6_add(even, aa, s);
  f12_join(r, even, cross);
}

// f^(p^6): odd w-coefficients negate (in place; validated by the generator)
__device__ inline void f12_conj6_ip(fp12m &a) {
  for (int k = 1; k < 6; k += 2) {
    fp2 c;
    f12_get(a, k, c);
    fp2_neg(c, c);
    f12_set(a, k, c);
  }
}

__device__ inline bool f12_is_one(const fp12m &a) {
  fp one;
  fp_one(one);
  if (!fp_eq(a.s[0], one)) return false;
  for (int i = 1; i < 12; i++)
    if (!fp_is_zero(a.s[i])) return false;
  return true;
}




// ---------------------------------------------------------------- pairing ---

// Per-pair constants of the inversion-free Miller loop. BOTH points stay
// JACOBIAN (no inversions anywhere; validated in Python). P side: lines
// are scaled by the Fp-subfield factor Zp^3 — a0 uses Yp directly, a3
// takes Zp^3, a5 uses Xp*Zp. Q side: addition lines carry the further
// subfield-norm factor Zq^3 via H* = X*Zq^2 - Xq*Z^2 (= H*Zq^2),
// M* = Y*Zq^3 - Yq*Z^3 (= M*Zq^3), with a0/a3 consuming H*Zq.
// Every line is additionally scaled by xi (instead of carrying xi^-1 in
// a3 and a5): a nonzero Fp2 factor lies in the Fp6 subfield and dies in
// the easy part of the final exponentiation, and xi*a0 is adds only.
struct miller_pre {
  fp xp, yp, zp3; // Xp*Zp, Yp, Zp^3
  fp2 zq2, zq3;   // Zq^2, Zq^3
};

__device__ inline void miller_precompute(miller_pre &c, const g1j &Pj,
                                         const g2j &Qj) {
  fp zp2;
  fp_sqr(zp2, Pj.z);
  fp_mul(c.zp3, zp2, Pj.z);
  fp_mul(c.xp, Pj.x, Pj.z);
  c.yp = Pj.y;
  fp2_sqr(c.zq2, Qj.z);
  fp2_mul(c.zq3, c.zq2, Qj.z);
}

// One doubling step: the tangent line at T evaluated at P, and T <- 2T.
// The line and the doubling (dbl-2009-l) share A = X^2, B = Y^2, E = 3A
// and Z3 = 2YZ:
//   a0 = xi * Z3*Z^2 * yp ; a3 = (E*X - 2B) * zp3 ; a5 = -E*Z^2 * xp
// (33 Fp mults against 28 + 16 for separate line and g2j_dbl).
__device__ inline void miller_dbl_step(g2j &T, fp2 &a0, fp2 &a3, fp2 &a5,
                                       const miller_pre &c) {
  fp2 A, B, C, D, E, F, Z2, Z3, t, t2;
  fp2_sqr(A, T.x);
  fp2_sqr(B, T.y);
  fp2_sqr(Z2, T.z);
  fp2_dbl(E, A);
  fp2_add(E, E, A);
  fp2_mul(t, T.y, T.z);
  fp2_dbl(Z3, t);
  fp2_mul(t, Z3, Z2);
  fp2_mul_fp(t, t, c.yp);
  fp2_mul_xi(a0, t);
  fp2_mul(t, E, T.x);
  fp2_dbl(t2, B);
  fp2_sub(t, t, t2);
  fp2_mul_fp(a3, t, c.zp3);
  fp2_mul(t, E, Z2);
  fp2_mul_fp(t, t, c.xp);
  fp2_neg(a5, t);
  fp2_sqr(C, B);
  fp2_add(D, T.x, B);
  fp2_sqr(D, D);
  fp2_sub(D, D, A);
  fp2_sub(D, D, C);
  fp2_dbl(D, D);
  fp2_sqr(F, E);
  fp2_sub(F, F, D);
  fp2_sub(F, F, D);
  fp2_sub(t, D, F);
  fp2_mul(t, E, t);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_sub(T.y, t, C);
  T.x = F;
  T.z = Z3;
}

// One addition step: the line through T and Q (both Jacobian) evaluated
// at P, scaled by Zq^3 and xi, and T <- T + Q:
//   a0 = xi * Z^3*H*Zq * yp ; a3 = (M**X - Y*H*Zq) * zp3 ;
//   a5 = -M**Z^2 * xp
__device__ inline void miller_add_step(g2j &T, fp2 &a0, fp2 &a3, fp2 &a5,
                                       const g2j &Qj, const miller_pre &c) {
  fp2 Z2, Z3, Hs, Ms, HZq, t, t2;
  fp2_sqr(Z2, T.z);
  fp2_mul(Z3, Z2, T.z);
  fp2_mul(t, T.x, c.zq2);
  fp2_mul(t2, Qj.x, Z2);
  fp2_sub(Hs, t, t2); // H* = H*Zq^2
  fp2_mul(t, T.y, c.zq3);
  fp2_mul(t2, Qj.y, Z3);
  fp2_sub(Ms, t, t2); // M* = M*Zq^3
  fp2_mul(HZq, Hs, Qj.z);
  fp2_mul(t, Z3, HZq);
  fp2_mul_fp(t, t, c.yp);
  fp2_mul_xi(a0, t);
  fp2_mul(t, Ms, T.x);
  fp2_mul(t2, T.y, HZq);
  fp2_sub(t, t, t2);
  fp2_mul_fp(a3, t, c.zp3);
  fp2_mul(t, Ms, Z2);
  fp2_mul_fp(t, t, c.xp);
  fp2_neg(a5, t);
  g2j_add(T, T, Qj);
}

// f <- f^2 * line for Miller iterations hi..lo of |x|: the shared body of
// miller_raw and miller_half. The tower square and the line product split
// their input out before writing, so f is updated in place and the loop
// needs no second Fp12 buffer.
__device__ inline void miller_iters(fp12m &f, g2j &T, const g2j &Qj,
                                    const miller_pre &c, int hi, int lo) {
  for (int i = hi; i >= lo; i--) {
    fp2 a0, a3, a5;
    f12_sqr_nn(f, f);
    miller_dbl_step(T, a0, a3, a5, c);
    f12_line_nn(f, f, a0, a3, a5);
    if ((BLS_X_ABS >> i) & 1) {
      miller_add_step(T, a0, a3, a5, Qj, c);
      f12_line_nn(f, f, a0, a3, a5);
    }
  }
}

// out = miller(P, Q) (already conjugated for x<0). Inversion-free Jacobian
// loop on the twist with sparse lines (formulas validated against the
// Python reference, tests/test_pairing_formulas_ref.py).
__device__ inline void miller_raw(fp12m &out, const g1j &Pj, const g2j &Qj) {
  f12_one(out);
  if (fp_is_zero(Pj.z) || fp2_is_zero(Qj.z)) return; // e(O,.) = e(.,O) = 1
  miller_pre c;
  miller_precompute(c, Pj, Qj);
  g2j T = Qj;
  miller_iters(out, T, Qj, c, 62, 0);
  f12_conj6_ip(out); // x < 0
}


// Half-Miller for the WAVE-SPLIT per-lane form (round 2): at the 64k-set
// C2 shape the per-lane Miller kernel is 1024 waves = 1 wave/SIMD —
// latency-exposed. Splitting each set across TWO waves (lane i = bits
// 62..32 + a 2^32 tail; lane n+i = bare T-chain then bits 31..0) doubles
// wave count to 2/SIMD and halves the per-lane dependent chain. Both
// roles are uniform per wave (no intra-wave divergence). Correctness:
// miller(P,Q) = f_hi^(2^32) * f_lo and conj6 distributes over the
// product, so the standard GT reduction of the 2n partials equals the
// reduction of n full Millers (validated vs the oracle verdicts).
// |x| = 0xd201000000010000: set bits {63,62,60,57,48,16} — the high half
// (i=62..32) carries 4 addition steps, the low half (i=31..0) one.
__device__ inline void miller_half(fp12m &out, const g1j &Pj, const g2j &Qj,
                                   int role) {
  f12_one(out);
  if (fp_is_zero(Pj.z) || fp2_is_zero(Qj.z)) return;
  miller_pre c;
  miller_precompute(c, Pj, Qj);
  g2j T = Qj;
  int lo = role == 0 ? 32 : 0;
  int hi = role == 0 ? 62 : 31;
  if (role == 1) {
    // bare T-chain over the high half (no f updates): ~1/4 of an
    // iteration's cost, so the duplicated chain is cheap
    for (int i = 62; i >= 32; i--) {
      g2j_dbl(T, T);
      if ((BLS_X_ABS >> i) & 1) g2j_add(T, T, Qj);
    }
  }
  miller_iters(out, T, Qj, c, hi, lo);
  if (role == 0) {
    // f_hi^(2^32): the tail squarings that align the high half with the
    // 32 low-half iterations it skipped
    for (int k = 0; k < 32; k++) f12_sqr_nn(out, out);
  }
  f12_conj6_ip(out); // x < 0 (conj6 distributes over the half product)
}


// ------------------------- wave-cooperative fp12 (64-thread finish path) ---
// All 64 lanes execute the same control flow; fp12 multiplies fan the 36
// coefficient products across lanes through an LDS staging area. Ops are
// ALIAS-SAFE (reads complete before the sync that precedes writes), so
// squarings and accumulations run in place. Requires blockDim.x == 64.

struct f12w_ws {
  fp2 t[36];
};

__device__ __forceinline__ void f12w_sync() { __syncthreads(); }

__device__ inline void f12_mul_w(fp12m &r, const fp12m &a, const fp12m &b,
                                 f12w_ws &ws, int lane) {
  if (lane < 36) {
    int i = lane / 6, j = lane % 6;
    // xi-weighting happens HERE (lane-parallel) and products land in
    // residue-grouped slots (class k=(i+j)%6 has exactly 6 entries at
    // k*6+i), so the fold is a short multi-lane tree: the old 6-lane
    // serial accumulate cost MORE than the whole 36-lane product phase
    // (12us vs 8.7us, tools/finishbench).
    fp2 ai, bj, t;
    f12_get(a, i, ai);
    f12_get(b, j, bj);
    fp2_mul(t, ai, bj);
    if (i + j >= 6) fp2_mul_xi(t, t);
    ws.t[((i + j) % 6) * 6 + i] = t;
  }
  f12w_sync();
  if (lane < 18) { // fold 6 -> 3 per class
    int k = lane / 3, pos = lane % 3;
    fp2 t0 = ws.t[k * 6 + pos], t1 = ws.t[k * 6 + pos + 3];
    fp2_add(t0, t0, t1);
    ws.t[k * 6 + pos] = t0;
  }
  f12w_sync();
  if (lane < 6) {
    fp2 acc, t;
    acc = ws.t[lane * 6];
    t = ws.t[lane * 6 + 1];
    fp2_add(acc, acc, t);
    t = ws.t[lane * 6 + 2];
    fp2_add(acc, acc, t);
    f12_set(r, lane, acc);
  }
  f12w_sync();
}

// f *= (a0 + a3 w^3 + a5 w^5), in place
__device__ inline void f12_line_w(fp12m &f, const fp2 &a0, const fp2 &a3,
                                  const fp2 &a5, f12w_ws &ws, int lane) {
  if (lane < 18) {
    // ONE uniform fp2_mul: per-branch multiplies would execute all three
    // bodies serially in the wave (see f12_sqr_w note)
    int k = lane / 3, q = lane % 3;
    int src = q == 0 ? k : (q == 1 ? (k + 3) % 6 : (k + 1) % 6);
    fp2 fk, coef, t;
    f12_get(f, src, fk);
    coef = q == 0 ? a0 : (q == 1 ? a3 : a5);
    fp2_mul(t, fk, coef);
    if ((q == 1 && k < 3) || (q == 2 && k < 5)) fp2_mul_xi(t, t);
    ws.t[lane] = t;
  }
  f12w_sync();
  if (lane < 6) {
    fp2 acc, t;
    acc = ws.t[3 * lane];
    t = ws.t[3 * lane + 1];
    fp2_add(acc, acc, t);
    t = ws.t[3 * lane + 2];
    fp2_add(acc, acc, t);
    f12_set(f, lane, acc);
  }
  f12w_sync();
}

__device__ inline void f12_copy_w(fp12m &r, const fp12m &a, int lane) {
  if (lane < 12) r.s[lane] = a.s[lane];
  f12w_sync();
}

__device__ inline void f12_conj6_w(fp12m &a, int lane) {
  if (lane < 3) {
    fp2 c;
    f12_get(a, 2 * lane + 1, c);
    fp2_neg(c, c);
    f12_set(a, 2 * lane + 1, c);
  }
  f12w_sync();
}

__device__ inline void f12_frob_w(fp12m &r, const fp12m &a, int power,
                                  int lane) {
  if (lane < 6) {
    fp2 fw1, fw, accw, c;
    FP2_LOAD_C(fw1, FROB_W1);
    if (power == 2) {
      fp2 c1;
      fp2_conj(c1, fw1);
      fp2_mul(fw, fw1, c1);
    } else {
      fw = fw1;
    }
    fp2_one(accw);
    for (int q = 0; q < lane; q++) fp2_mul(accw, accw, fw);
    f12_get(a, lane, c);
    if (power == 1) fp2_conj(c, c);
    fp2_mul(c, c, accw);
    f12_set(r, lane, c);
  }
  f12w_sync();
}

// r = a^-1; r, g, t distinct from a and each other
__device__ inline void f12_inv_w(fp12m &r, const fp12m &a, fp12m &g, fp12m &t,
                                 f12w_ws &ws, int lane) {
  if (lane == 0) f12_one(g);
  f12w_sync();
  for (int i = 1; i < 6; i++) {
    if (lane < 6) {
      fp2 z6, zi, fac, c;
      FP2_LOAD_C(z6, ZETA6);
      fp2_one(zi);
      for (int q = 0; q < i; q++) fp2_mul(zi, zi, z6);
      fp2_one(fac);
      for (int q = 0; q < lane; q++) fp2_mul(fac, fac, zi);
      f12_get(a, lane, c);
      fp2_mul(c, c, fac);
      f12_set(t, lane, c);
    }
    f12w_sync();
    f12_mul_w(g, g, t, ws, lane); // in-place safe
  }
  f12_mul_w(t, a, g, ws, lane); // norm in t.c0
  if (lane == 0) {
    fp2 n0, ninv;
    f12_get(t, 0, n0);
    fp2_inv(ninv, n0);
    ws.t[0] = ninv;
  }
  f12w_sync();
  if (lane < 6) {
    fp2 c, ninv = ws.t[0];
    f12_get(g, lane, c);
    fp2_mul(c, c, ninv);
    f12_set(r, lane, c);
  }
  f12w_sync();
}

// cooperative squaring: 21 distinct products across lanes (alias-safe)
// residue-grouped slot map for the cooperative squaring fold: product
// qi (pi<=pj enumeration) lands at slot ((pi+pj)%6)*4 + pos; groups have
// 3 or 4 entries, pads (slots 7, 15, 23) are zeroed by lanes 21-23.
// Doubling (pi!=pj) and xi-weighting (pi+pj>=6) are applied in the
// product phase.
__constant__ int F12_SQR_SLOT[21] = {0, 4,  8,  12, 16, 20, 9, 13, 17,
                                     21, 1, 18, 22, 2,  5,  3, 6,  10,
                                     11, 14, 19};
__constant__ int F12_SQR_PI[21] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1,
                                   2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
__constant__ int F12_SQR_PJ[21] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5,
                                   2, 3, 4, 5, 3, 4, 5, 4, 5, 5};

__device__ inline void f12_sqr_w(fp12m &a, f12w_ws &ws, int lane) {
  int li = lane < 21 ? lane : 0;
  int i = F12_SQR_PI[li];
  int j = F12_SQR_PJ[li];
  if (lane < 21) {
    // UNIFORM fp2_mul even on the diagonal (a divergent fp2_sqr branch
    // would execute both bodies); doubling + xi-weighting lane-parallel
    // here; residue-grouped slots so the fold is a 2-step tree — the old
    // 21-entry 6-lane scan was ~27us, 3x the product phase.
    fp2 ai, aj, t;
    f12_get(a, i, ai);
    f12_get(a, j, aj);
    fp2_mul(t, ai, aj);
    if (i != j) fp2_dbl(t, t);
    if (i + j >= 6) fp2_mul_xi(t, t);
    ws.t[F12_SQR_SLOT[lane]] = t;
  } else if (lane < 24) { // zero the pad slots 7, 15, 23
    fp2 z;
    fp2_zero(z);
    ws.t[8 * (lane - 21) + 7] = z;
  }
  f12w_sync();
  if (lane < 12) { // fold 4 -> 2 per class
    int k = lane / 2, pos = lane % 2;
    fp2 t0 = ws.t[k * 4 + pos], t1 = ws.t[k * 4 + pos + 2];
    fp2_add(t0, t0, t1);
    ws.t[k * 4 + pos] = t0;
  }
  f12w_sync();
  if (lane < 6) {
    fp2 acc, t;
    acc = ws.t[lane * 4];
    t = ws.t[lane * 4 + 1];
    fp2_add(acc, acc, t);
    f12_set(a, lane, acc);
  }
  f12w_sync();
}


// cyclotomic squaring (Granger-Scott), cooperative — valid ONLY for
// elements of the cyclotomic subgroup (anything after the easy part,
// i.e. every final-exp pow-chain input). 9 fp2 squarings across lanes
// (vs 21 products in f12_sqr_w); the three Fp4 = Fp2[w^3] subalgebras
// (g0,g3) (g1,g4) (g2,g5) are squared and recombined as
//   h_even = 3*t0 - 2*g_even,  h_odd = 3*cross(*xi for h1) + 2*g_odd.
// Formulas validated against the generic squaring on random cyclotomic
// elements in Python (see round-2 session notes / DESIGN.md).
__constant__ int F12_CYC_OUT[6] = {0, 3, 2, 5, 4, 1};
__constant__ int F12_CYC_PAIR[6] = {0, 0, 1, 1, 2, 2};
__constant__ int F12_CYC_KIND[6] = {0, 1, 0, 1, 0, 1}; // 0 = t0, 1 = cross

__device__ inline void f12_sqr_cyc_w(fp12m &a, f12w_ws &ws, int lane) {
  if (lane < 9) {
    int pair = lane / 3, which = lane % 3;
    fp2 a0, a1, v, sq;
    f12_get(a, pair, a0);
    f12_get(a, pair + 3, a1);
    if (which == 0)
      v = a0;
    else if (which == 1)
      v = a1;
    else
      fp2_add(v, a0, a1);
    fp2_sqr(sq, v);
    ws.t[lane] = sq;
  }
  f12w_sync();
  if (lane < 6) {
    int out = F12_CYC_OUT[lane];
    int pr = F12_CYC_PAIR[lane];
    fp2 s0 = ws.t[3 * pr], s1 = ws.t[3 * pr + 1], ss = ws.t[3 * pr + 2];
    fp2 t, h, gcur;
    f12_get(a, out, gcur);
    if (F12_CYC_KIND[lane] == 0) {
      fp2_mul_xi(t, s1);
      fp2_add(t, t, s0); /* t0 = a0^2 + xi*a1^2 */
      fp2 t3;
      fp2_dbl(t3, t);
      fp2_add(t3, t3, t); /* 3*t0 */
      fp2_dbl(gcur, gcur);
      fp2_sub(h, t3, gcur); /* 3*t0 - 2*g */
    } else {
      fp2_sub(t, ss, s0);
      fp2_sub(t, t, s1); /* cross = 2*a0*a1 */
      if (out == 1) fp2_mul_xi(t, t);
      fp2 t3;
      fp2_dbl(t3, t);
      fp2_add(t3, t3, t); /* 3*cross */
      fp2_dbl(gcur, gcur);
      fp2_add(h, t3, gcur); /* 3*cross + 2*g */
    }
    ws.t[18 + lane] = h; /* stage outputs (a still being read) */
  }
  f12w_sync();
  if (lane < 6) {
    int out = F12_CYC_OUT[lane];
    f12_set(a, out, ws.t[18 + lane]);
  }
  f12w_sync();
}

// r = a^|x|; r distinct from a. a and all intermediates are cyclotomic
// here (final-exp chains), so the Granger-Scott squaring applies.
__device__ inline void f12_pow_xabs_w(fp12m &r, const fp12m &a, f12w_ws &ws,
                                      int lane) {
  f12_copy_w(r, a, lane);
  for (int b = 62; b >= 0; b--) {
    f12_sqr_cyc_w(r, ws, lane);
    if ((BLS_X_ABS >> b) & 1) f12_mul_w(r, r, a, ws, lane);
  }
}

// cooperative miller workspace: the 68 per-step line-coefficient records
// (63 doublings + 5 additions for |x| = 0xd201000000010000)
struct miller_ws {
  fp2 T[68][3];    // T (Jacobian) BEFORE each step
  fp2 coef[68][3]; // line (a0, a3, a5) per step
};

// out = miller(P, Q) (conjugated), one wave. Three phases: (1) the serial
// T-chain (lane 0) storing pre-step points, (2) line coefficients for all
// steps computed in PARALLEL across lanes, (3) the f-chain with
// cooperative fp12 ops consuming the stored coefficients.
__device__ inline void miller_w(fp12m &out, const g1j &Pj, const g2j &Qj,
                                f12w_ws &ws, miller_ws &mws, int lane) {
  if (lane == 0) f12_one(out);
  f12w_sync();
  if (fp_is_zero(Pj.z) || fp2_is_zero(Qj.z)) return;
  fp2 xi_inv; // constant (1-u)/2
  FP_LOAD_C(xi_inv.c0, FP_TWO_INV);
  fp_neg(xi_inv.c1, xi_inv.c0);
  // BOTH points Jacobian (as miller_raw; validated in Python). P side:
  // lines scaled by Zp^3 (a0 <- Yp, a3's xi^-1 absorbs Zp^3, a5 <- Xp*Zp).
  // Q side: addition lines carry the further subfield-norm factor Zq^3
  // (H* / M* / H*Zq form). Wave-uniform values, computed redundantly.
  fp2 zq2, zq3, xi_inv_zp3;
  fp2_sqr(zq2, Qj.z);
  fp2_mul(zq3, zq2, Qj.z);
  fp zp2, zp3, xp, yp;
  fp_sqr(zp2, Pj.z);
  fp_mul(zp3, zp2, Pj.z);
  fp_mul(xp, Pj.x, Pj.z);
  yp = Pj.y;
  fp2_mul_fp(xi_inv_zp3, xi_inv, zp3);
  // ---- phase 1: serial point chain (lane 0 writes pre-step T) ----
  if (lane == 0) {
    g2j T = Qj;
    int idx = 0;
    for (int i = 62; i >= 0; i--) {
      mws.T[idx][0] = T.x;
      mws.T[idx][1] = T.y;
      mws.T[idx][2] = T.z;
      idx++;
      g2j_dbl(T, T);
      if ((BLS_X_ABS >> i) & 1) {
        mws.T[idx][0] = T.x;
        mws.T[idx][1] = T.y;
        mws.T[idx][2] = T.z;
        idx++;
        g2j_add(T, T, Qj);
      }
    }
  }
  f12w_sync();
  // ---- phase 2: lanes compute the 68 line-coefficient records in
  // parallel (68 > 64 lanes: strided, lanes 0-3 take a second record) ----
  for (int rec = lane; rec < 68; rec += 64) {
    // derive this record's kind (doubling or addition) from the fixed
    // step pattern of |x|
    int idx = 0;
    int my_kind = -1;
    for (int i = 62; i >= 0 && my_kind < 0; i--) {
      if (idx == rec) my_kind = 0; // doubling record
      idx++;
      if ((BLS_X_ABS >> i) & 1) {
        if (my_kind < 0 && idx == rec) my_kind = 1; // addition record
        idx++;
      }
    }
    g2j T;
    T.x = mws.T[rec][0];
    T.y = mws.T[rec][1];
    T.z = mws.T[rec][2];
    fp2 a0, a3, a5, t, t2;
    if (my_kind == 0) {
      fp2 X2, Y2, Z2, Z3;
      fp2_sqr(X2, T.x);
      fp2_sqr(Y2, T.y);
      fp2_sqr(Z2, T.z);
      fp2_mul(Z3, Z2, T.z);
      fp2_mul(t, T.y, Z3);
      fp2_dbl(t, t);
      fp2_mul_fp(a0, t, yp);
      fp2_mul(t, X2, T.x);
      fp2_mul_small(t, t, 3);
      fp2_dbl(t2, Y2);
      fp2_sub(t, t, t2);
      fp2_mul(a3, t, xi_inv_zp3);
      fp2_mul(t, X2, Z2);
      fp2_mul_small(t, t, 3);
      fp2_mul_fp(t, t, xp);
      fp2_neg(t, t);
      fp2_mul(a5, t, xi_inv);
    } else {
      fp2 Z2, Z3, Hs, Ms, HZq;
      fp2_sqr(Z2, T.z);
      fp2_mul(Z3, Z2, T.z);
      fp2_mul(t, T.x, zq2);
      fp2_mul(t2, Qj.x, Z2);
      fp2_sub(Hs, t, t2); // H* = H*Zq^2
      fp2_mul(t, T.y, zq3);
      fp2_mul(t2, Qj.y, Z3);
      fp2_sub(Ms, t, t2); // M* = M*Zq^3
      fp2_mul(HZq, Hs, Qj.z);
      fp2_mul(t, Z3, HZq);
      fp2_mul_fp(a0, t, yp);
      fp2_mul(t, Ms, T.x);
      fp2_mul(t2, T.y, HZq);
      fp2_sub(t, t, t2);
      fp2_mul(a3, t, xi_inv_zp3);
      fp2_mul(t, Ms, Z2);
      fp2_mul_fp(t, t, xp);
      fp2_neg(t, t);
      fp2_mul(a5, t, xi_inv);
    }
    mws.coef[rec][0] = a0;
    mws.coef[rec][1] = a3;
    mws.coef[rec][2] = a5;
  }
  f12w_sync();
  // ---- phase 3: the f-chain over stored coefficients ----
  {
    int idx = 0;
    for (int i = 62; i >= 0; i--) {
      f12_sqr_w(out, ws, lane);
      f12_line_w(out, mws.coef[idx][0], mws.coef[idx][1], mws.coef[idx][2],
                 ws, lane);
      idx++;
      if ((BLS_X_ABS >> i) & 1) {
        f12_line_w(out, mws.coef[idx][0], mws.coef[idx][1], mws.coef[idx][2],
                   ws, lane);
        idx++;
      }
    }
  }
  f12_conj6_w(out, lane);
}

// r = final_exp(f); r, f distinct from the 4 scratch slots s[0..3]
__device__ inline void final_exp_w(fp12m &r, const fp12m &f, fp12m *s,
                                   f12w_ws &ws, int lane) {
  f12_copy_w(s[0], f, lane);
  f12_conj6_w(s[0], lane); // f^(p^6)
  f12_inv_w(s[1], f, s[2], s[3], ws, lane);
  f12_mul_w(s[1], s[0], s[1], ws, lane); // f^(p^6-1)
  f12_frob_w(s[0], s[1], 2, lane);
  f12_mul_w(s[1], s[0], s[1], ws, lane); // e (cyclotomic)
  f12_pow_xabs_w(s[0], s[1], ws, lane);  // e^|x|
  f12_mul_w(s[0], s[0], s[1], ws, lane);
  f12_conj6_w(s[0], lane); // u = e^(x-1)
  f12_pow_xabs_w(s[2], s[0], ws, lane);
  f12_mul_w(s[2], s[2], s[0], ws, lane);
  f12_conj6_w(s[2], lane); // v = e^((x-1)^2)
  f12_pow_xabs_w(s[3], s[2], ws, lane);
  f12_conj6_w(s[3], lane); // v^x
  f12_frob_w(s[0], s[2], 1, lane);
  f12_mul_w(s[3], s[3], s[0], ws, lane); // w1 = v^(x+p)
  f12_pow_xabs_w(s[0], s[3], ws, lane);
  f12_conj6_w(s[0], lane); // w1^x
  f12_pow_xabs_w(s[2], s[0], ws, lane);
  f12_conj6_w(s[2], lane); // w1^(x^2)
  f12_frob_w(s[0], s[3], 2, lane);
  f12_mul_w(s[2], s[2], s[0], ws, lane);
  f12_copy_w(s[0], s[3], lane);
  f12_conj6_w(s[0], lane);
  f12_mul_w(s[2], s[2], s[0], ws, lane); // w2
  f12_mul_w(s[0], s[1], s[1], ws, lane); // e^2
  f12_mul_w(s[0], s[0], s[1], ws, lane); // e^3
  f12_mul_w(r, s[2], s[0], ws, lane);
}

// --------------------------------------------------------- hash-to-curve ---

__device__ inline void h2f_from_be64(fp &r, const uint8_t *b) {
  // 64-byte BE -> Fp (mod p): hi*2^384 + lo
  uint64_t lo[6], hi2[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w = (w << 8) | b[16 + 8 * i + j];
    lo[5 - i] = w;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) hi2[i] = 0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w = (w << 8) | b[8 * i + j];
    hi2[1 - i] = w;
  }
  while (fp_ge_p(lo)) fp_sub_p(lo);
  fp hif, r2, hi384;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    hif.v[i] = hi2[i];
    r2.v[i] = BLS_R2[i];
  }
  fp_mul(hi384, hif, r2); // hi*R (standard form)
  uint64_t sum[6];
  unsigned __int128 c = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    c += (unsigned __int128)hi384.v[i] + lo[i];
    sum[i] = (uint64_t)c;
    c >>= 64;
  }
  if (c || fp_ge_p(sum)) fp_sub_p(sum);
  fp_from_std(r, sum);
}

__device__ inline void expand_message_xmd32(const uint8_t *msg,
                                            uint8_t out[256]) {
  // DST = blst.rs:15 (43 bytes); msg_len = 32; len_in_bytes = 256, ell = 8
  const char DSTs[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
  const int dst_len = 43;
  uint8_t buf[64 + 32 + 2 + 1 + 44];
  int off = 0;
  for (int i = 0; i < 64; i++) buf[off++] = 0;
  for (int i = 0; i < 32; i++) buf[off++] = msg[i];
  buf[off++] = 1;
  buf[off++] = 0;
  buf[off++] = 0;
  for (int i = 0; i < dst_len; i++) buf[off++] = (uint8_t)DSTs[i];
  buf[off++] = (uint8_t)dst_len;
  uint8_t b0[32];
  m3x::sha256_bytes(buf, off, b0);
  uint8_t cur[32 + 1 + 44];
  for (int i = 0; i < 32; i++) cur[i] = b0[i];
  cur[32] = 1;
  for (int i = 0; i < dst_len; i++) cur[33 + i] = (uint8_t)DSTs[i];
  cur[33 + dst_len] = (uint8_t)dst_len;
  uint8_t bi[32];
  m3x::sha256_bytes(cur, 33 + dst_len + 1, bi);
  for (int i = 0; i < 32; i++) out[i] = bi[i];
  for (int blk = 2; blk <= 8; blk++) {
    for (int j = 0; j < 32; j++) cur[j] = b0[j] ^ bi[j];
    cur[32] = (uint8_t)blk;
    m3x::sha256_bytes(cur, 33 + dst_len + 1, bi);
    for (int j = 0; j < 32; j++) {
      bi[j] = bi[j];
      out[32 * (blk - 1) + j] = bi[j];
    }
  }
}

// General-DST expand_message_xmd (RFC 9380 §5.3.1, SHA-256): test-entry
// form for the external RFC vectors (tests/golden/rfc9380_vectors.json);
// the hot path keeps the fixed-DST expand_message_xmd32 below.
__device__ inline void expand_message_xmd_gen(const uint8_t *msg,
                                              uint32_t msg_len,
                                              const uint8_t *dst,
                                              uint32_t dst_len,
                                              uint32_t len_in_bytes,
                                              uint8_t *out) {
  uint32_t ell = (len_in_bytes + 31) / 32;
  uint8_t buf[64 + 544 + 2 + 1 + 255 + 1];
  uint32_t off = 0;
  for (int i = 0; i < 64; i++) buf[off++] = 0;
  for (uint32_t i = 0; i < msg_len; i++) buf[off++] = msg[i];
  buf[off++] = (uint8_t)(len_in_bytes >> 8);
  buf[off++] = (uint8_t)len_in_bytes;
  buf[off++] = 0;
  for (uint32_t i = 0; i < dst_len; i++) buf[off++] = dst[i];
  buf[off++] = (uint8_t)dst_len;
  uint8_t b0[32];
  m3x::sha256_bytes(buf, off, b0);
  uint8_t cur[32 + 1 + 255 + 1];
  for (int i = 0; i < 32; i++) cur[i] = b0[i];
  cur[32] = 1;
  for (uint32_t i = 0; i < dst_len; i++) cur[33 + i] = dst[i];
  cur[33 + dst_len] = (uint8_t)dst_len;
  uint8_t bi[32];
  m3x::sha256_bytes(cur, 33 + dst_len + 1, bi);
  uint32_t copied = len_in_bytes < 32 ? len_in_bytes : 32;
  for (uint32_t i = 0; i < copied; i++) out[i] = bi[i];
  for (uint32_t blk = 2; blk <= ell; blk++) {
    for (int j = 0; j < 32; j++) cur[j] = b0[j] ^ bi[j];
    cur[32] = (uint8_t)blk;
    m3x::sha256_bytes(cur, 33 + dst_len + 1, bi);
    uint32_t base = 32 * (blk - 1);
    uint32_t nc = len_in_bytes - base < 32 ? len_in_bytes - base : 32;
    for (uint32_t i = 0; i < nc; i++) out[base + i] = bi[i];
  }
}

// SSWU by the definition, with a real inversion: only for the exceptional
// inputs sswu_g2 hands over (never data-typical). Out of line and entered
// only after sswu_g2_fast has returned, so its frames (fp2_sqrt, fp2_inv)
// do not stack on top of the fast path's.
__device__ __noinline__ void sswu_g2_slow(g2a &out, const fp2 &u) {
  fp2 A, B, Z, zu2, tv, x1, gx, y, t;
  FP2_LOAD_C(A, SSWU_A);
  FP2_LOAD_C(B, SSWU_B);
  FP2_LOAD_C(Z, SSWU_Z);
  fp2_sqr(zu2, u);
  fp2_mul(zu2, zu2, Z);
  fp2_sqr(tv, zu2);
  fp2_add(tv, tv, zu2);
  if (fp2_is_zero(tv)) {
    FP2_LOAD_C(x1, SSWU_B_DIV_ZA); // constant B/(Z*A)
  } else {
    fp2 nb_over_a, one;
    FP2_LOAD_C(nb_over_a, SSWU_NB_DIV_A); // constant -B/A
    fp2_inv(t, tv);
    fp2_one(one);
    fp2_add(t, t, one);
    fp2_mul(x1, nb_over_a, t);
  }
#pragma unroll 1
  for (int c = 0; c < 2; c++) { // x1, then x2 = Z u^2 x1
    fp2_sqr(gx, x1);
    fp2_add(gx, gx, A);
    fp2_mul(gx, gx, x1);
    fp2_add(gx, gx, B);
    if (fp2_sqrt(y, gx)) break;
    fp2_mul(x1, zu2, x1);
  }
  if (fp2_sgn0(u) != fp2_sgn0(y)) fp2_neg(y, y);
  out.x = x1;
  out.y = y;
  out.inf = 0;
}

// Simplified SWU onto E2' with exactly TWO pow chains per point, no
// inversion, no retry, and the same control flow in every lane
// (tests/h2c_sqrt_ref.py restates it over exact integers):
//  * projective x1 = xn/xd, xn = B(tv+1), xd = -A tv (Z A when tv = 0);
//    a = gn xd = g(x1) xd^4 has the squareness of g(x1)
//  * pow 1, u1 = N(a)^((p-3)/4): s1 = u1 N(a) is the norm's root when
//    s1^2 = N(a) (g(x1) square), and 1/N(a) = +-u1^2 by that same test,
//    whence 1/xd = conj(xd) N(gn)/N(a)
//  * when the test fails s1^2 = -N(a), and since N(Z) = 5 with -5 a residue,
//    sqrt N(zu2^3 a) = N(zu2) N(u) sqrt(-5) s1: the norm root for the
//    second candidate g(x2) xd^4 = zu2^3 a comes for free
//  * pow 2 inside fp2_sqrt_from_norm_root; y = root/xd^2
// Returns false, out untouched, for the exceptional inputs.
__device__ __noinline__ bool sswu_g2_fast(g2a &out, const fp2 &u) {
  fp2 A, B, Z, zu2, tv, xn, xd, a, t;
  fp ng, nzu, n;
  FP2_LOAD_C(A, SSWU_A);
  FP2_LOAD_C(B, SSWU_B);
  FP2_LOAD_C(Z, SSWU_Z);
  fp2_sqr(zu2, u);
  fp2_mul(zu2, zu2, Z);
  fp2_sqr(tv, zu2);
  fp2_add(tv, tv, zu2);
  {
    fp2 one, za, xd2, gn;
    fp2_one(one);
    fp2_add(xn, tv, one);
    fp2_mul(xn, xn, B);
    fp2_mul(xd, A, tv);
    fp2_neg(xd, xd);
    fp2_mul(za, Z, A);
    fp2_sel(xd, fp2_is_zero(tv), za, xd);
    fp2_sqr(xd2, xd);
    fp2_sqr(gn, xn);
    fp2_mul(t, A, xd2);
    fp2_add(gn, gn, t);
    fp2_mul(gn, gn, xn);
    fp2_mul(t, xd2, xd);
    fp2_mul(t, t, B);
    fp2_add(gn, gn, t); // xn^3 + A xn xd^2 + B xd^3
    fp2_mul(a, gn, xd);
    fp2_norm(ng, gn);
    fp nu;
    fp2_norm(nzu, zu2);
    fp2_norm(nu, u);
    fp_mul(nzu, nzu, nu); // N(zu2) N(u)
  }
  fp2_norm(n, a);
  fp u1, s1, chk;
  fp_pow_m3(u1, n);
  fp_mul(s1, u1, n);
  fp_sqr(chk, s1);
  bool is_sq = fp_eq(chk, n); // g(x1) is a square
  fp2 sel;
  fp s;
  {
    fp2 a2;
    fp c5, s2;
    fp2_sqr(t, zu2);
    fp2_mul(t, t, zu2);
    fp2_mul(a2, t, a); // g(x2) xd^4
    FP_LOAD_C(c5, FP_SQRT_NEG5);
    fp_mul(s2, nzu, c5);
    fp_mul(s2, s2, s1);
    fp2_sel(sel, is_sq, a, a2);
    fp_sel(s, is_sq, s1, s2);
  }
  // g(x1) = 0, or the root's d = 0: never data-typical
  if (fp_is_zero(n) || fp_is_zero(sel.c1)) return false;
  // x and 1/xd^2 before the second pow, so little stays live across it
  fp2 x, xdi2;
  {
    fp ninv, nn, k;
    fp2 xdi, xz;
    fp_sqr(ninv, u1);
    fp_neg(nn, ninv);
    fp_sel(ninv, is_sq, ninv, nn); // 1/N(a)
    fp_mul(k, ng, ninv);           // 1/N(xd)
    fp2_conj(xdi, xd);
    fp2_mul_fp(xdi, xdi, k); // 1/xd
    fp2_mul(x, xn, xdi);
    fp2_mul(xz, x, zu2);
    fp2_sel(x, is_sq, x, xz);
    fp2_sqr(xdi2, xdi);
  }
  fp2 root, y;
  fp2_sqrt_from_norm_root(root, sel, s);
  fp2_mul(y, root, xdi2);
  if (fp2_sgn0(u) != fp2_sgn0(y)) fp2_neg(y, y);
  out.x = x;
  out.y = y;
  out.inf = 0;
  return true;
}

__device__ __forceinline__ void sswu_g2(g2a &out, const fp2 &u) {
  if (!sswu_g2_fast(out, u)) sswu_g2_slow(out, u);
}

// iso_map emitting JACOBIAN coordinates — no inversion at all:
// x = xn/xd, y = in.y*yn/yd maps to Z = xd*yd, X = xn*xd*yd^2,
// Y = in.y*yn*yd^2*xd^3 (X/Z^2 = xn/xd, Y/Z^3 = in.y*yn/yd).
__device__ inline void iso_map_g2_j(g2j &out, const g2a &in) {
  fp2 k[4], xn, xd, yn, yd;
  FP2_LOAD_C(k[0], ISO_XNUM0);
  FP2_LOAD_C(k[1], ISO_XNUM1);
  FP2_LOAD_C(k[2], ISO_XNUM2);
  FP2_LOAD_C(k[3], ISO_XNUM3);
  xn = k[3];
  for (int i = 2; i >= 0; i--) {
    fp2_mul(xn, xn, in.x);
    fp2_add(xn, xn, k[i]);
  }
  FP2_LOAD_C(k[0], ISO_XDEN0);
  FP2_LOAD_C(k[1], ISO_XDEN1);
  FP2_LOAD_C(k[2], ISO_XDEN2);
  xd = k[2];
  for (int i = 1; i >= 0; i--) {
    fp2_mul(xd, xd, in.x);
    fp2_add(xd, xd, k[i]);
  }
  FP2_LOAD_C(k[0], ISO_YNUM0);
  FP2_LOAD_C(k[1], ISO_YNUM1);
  FP2_LOAD_C(k[2], ISO_YNUM2);
  FP2_LOAD_C(k[3], ISO_YNUM3);
  yn = k[3];
  for (int i = 2; i >= 0; i--) {
    fp2_mul(yn, yn, in.x);
    fp2_add(yn, yn, k[i]);
  }
  FP2_LOAD_C(k[0], ISO_YDEN0);
  FP2_LOAD_C(k[1], ISO_YDEN1);
  FP2_LOAD_C(k[2], ISO_YDEN2);
  FP2_LOAD_C(k[3], ISO_YDEN3);
  yd = k[3];
  for (int i = 2; i >= 0; i--) {
    fp2_mul(yd, yd, in.x);
    fp2_add(yd, yd, k[i]);
  }
  fp2 yd2, xd2, xd3, t;
  fp2_sqr(yd2, yd);
  fp2_sqr(xd2, xd);
  fp2_mul(xd3, xd2, xd);
  fp2_mul(out.z, xd, yd);
  fp2_mul(t, xn, xd);
  fp2_mul(out.x, t, yd2);
  fp2_mul(t, yd2, xd3);
  fp2_mul(t, t, yn);
  fp2_mul(out.y, t, in.y);
}

__device__ inline void g2j_neg(g2j &r, const g2j &p) {
  r.x = p.x;
  fp2_neg(r.y, p.y);
  r.z = p.z;
}

// psi on Jacobian coordinates: psi(X,Y,Z) = (cx*conj(X), cy*conj(Y),
// conj(Z)) — X'/Z'^2 = cx*conj(X/Z^2), Y'/Z'^3 = cy*conj(Y/Z^3); no
// inversion needed.
__device__ inline void psi_g2j(g2j &r, const g2j &p) {
  fp2 cx, cy, t;
  FP2_LOAD_C(cx, PSI_CX);
  FP2_LOAD_C(cy, PSI_CY);
  fp2_conj(t, p.x);
  fp2_mul(r.x, t, cx);
  fp2_conj(t, p.y);
  fp2_mul(r.y, t, cy);
  fp2_conj(r.z, p.z);
}

// [k]P with a Jacobian base (the few additions use the full add)
__device__ inline void g2j_mul_u64_j(g2j &r, const g2j &base, uint64_t k) {
  g2j acc;
  g2j_set_inf(acc);
  for (int b = 63; b >= 0; b--) {
    g2j_dbl(acc, acc);
    if ((k >> b) & 1) g2j_add(acc, acc, base);
  }
  r = acc;
}

__device__ inline void clear_cofactor_g2j(g2j &out, const g2j &p) {
  // Budroni-Pintore (== RFC h_eff; validated by generator), fully
  // inversion-free in Jacobian coordinates.
  g2j xp, xxp, acc, tmp, d;
  g2j_mul_u64_j(xp, p, BLS_X_ABS);
  g2j_neg(xp, xp); // [x]P
  g2j_mul_u64_j(xxp, xp, BLS_X_ABS);
  g2j_neg(xxp, xxp); // [x^2]P
  acc = xxp;
  g2j_neg(tmp, xp);
  g2j_add(acc, acc, tmp);
  g2j_neg(tmp, p);
  g2j_add(acc, acc, tmp); // [x^2-x-1]P
  d = xp;
  g2j_neg(tmp, p);
  g2j_add(d, d, tmp);
  psi_g2j(tmp, d);
  g2j_add(acc, acc, tmp); // + [x-1]psi(P)
  g2j_dbl(tmp, p);
  psi_g2j(tmp, tmp);
  psi_g2j(tmp, tmp);
  g2j_add(acc, acc, tmp); // + psi^2([2]P)
  out = acc;
}

__device__ inline void h2c_g2_from_uniform(g2j &r, const uint8_t uni[256]) {
  fp2 u[2];
  h2f_from_be64(u[0].c0, uni);
  h2f_from_be64(u[0].c1, uni + 64);
  h2f_from_be64(u[1].c0, uni + 128);
  h2f_from_be64(u[1].c1, uni + 192);
  g2j pt[2];
#pragma unroll 1
  for (int i = 0; i < 2; i++) {
    g2a q;
    sswu_g2(q, u[i]);          // two pows, no inversion to share
    iso_map_g2_j(pt[i], q);    // Jacobian iso: no inversion at all
  }
  g2j s;
  g2j_add(s, pt[0], pt[1]);
  clear_cofactor_g2j(r, s); // stays Jacobian: consumers (Q-Jacobian
                            // Miller loops) need no inversion at all
}

__device__ inline void h2c_g2(g2j &r, const uint8_t *msg) {
  uint8_t uni[256];
  expand_message_xmd32(msg, uni);
  h2c_g2_from_uniform(r, uni);
}

// affine G2 -> 192B uncompressed wire form (x.c1||x.c0||y.c1||y.c0 BE)
__device__ inline void g2_to_uncomp_dev(const g2a &p, uint8_t *out) {
  fp_to_be48(p.x.c1, out);
  fp_to_be48(p.x.c0, out + 48);
  fp_to_be48(p.y.c1, out + 96);
  fp_to_be48(p.y.c0, out + 144);
}

// G1 generator (negated y variant computed by callers when needed)
__device__ inline void g1_gen(g1a &g) {
  FP_LOAD_C(g.x, BLS_G1X);
  FP_LOAD_C(g.y, BLS_G1Y);
  g.inf = 0;
}

// ------------------------------------------------------- block reductions ---

// LDS halving tree: folds lds[0..W) into lds[0] with op(r, a, b), r distinct
// from a and b. Thread t has just stored lds[t]; the leading barrier
// publishes those stores and each level ends with one, so lds[0] is visible
// to every thread on return. A caller that reuses lds afterwards (a
// grid-stride loop) still needs its own barrier after reading lds[0].
template <typename T, int W, typename Op>
__device__ __forceinline__ void block_tree_reduce(T *lds, int t, Op op) {
  __syncthreads();
  for (int s = W / 2; s > 0; s >>= 1) {
    if (t < s) {
      T r;
      op(r, lds[t], lds[t + s]);
      lds[t] = r;
    }
    __syncthreads();
  }
}

// the two point sums as combine functors
struct g1j_add_op {
  __device__ __forceinline__ void operator()(g1j &r, const g1j &a,
                                             const g1j &b) const {
    g1j_add(r, a, b);
  }
};
struct g2j_add_op {
  __device__ __forceinline__ void operator()(g2j &r, const g2j &a,
                                             const g2j &b) const {
    g2j_add(r, a, b);
  }
};

// One stage of a two-stage reduction: the block folds its contiguous span of
// in[0..n) (thread-strided local fold, then the LDS tree) into
// out[blockIdx.x]; a second one-block launch folds the partials. A thread
// starts from its first element (no fold with the identity); only a thread
// with no element takes ident(local). op(r, a, b) may be called with r == a.
template <typename T, int W, typename Op, typename Ident>
__device__ __forceinline__ void block_span_reduce(const T *__restrict__ in,
                                                  uint64_t n,
                                                  T *__restrict__ out, T *lds,
                                                  Op op, Ident ident) {
  uint64_t per = (n + gridDim.x - 1) / gridDim.x;
  uint64_t lo = (uint64_t)blockIdx.x * per;
  uint64_t hi = lo + per < n ? lo + per : n;
  T local;
  uint64_t i = lo + threadIdx.x;
  if (i < hi) {
    local = in[i];
    for (i += W; i < hi; i += W) op(local, local, in[i]);
  } else {
    ident(local);
  }
  lds[threadIdx.x] = local;
  block_tree_reduce<T, W>(lds, (int)threadIdx.x, op);
  if (threadIdx.x == 0) out[blockIdx.x] = lds[0];
}

} // namespace m3xb
