// What the KZG translation units share (internal): the setup handle, the
// per-lane G1 helpers, and launchers for the kernels of m3x_kzg.hip that the
// cell pipeline (m3x_kzg_cells.hip) reuses.
//
// The kernels themselves stay in m3x_kzg.hip and are reached through the
// launchers below, the way m3x_bls_each.hip is reached from m3x_bls.hip: one
// compiled copy, and the blob pipeline's kernels compile exactly as before.
#pragma once
#include "bls_device.hh"
#include "m3x_ctx.hh"

// affine entry of a fixed-base table; no entry is infinity (d * 2^(4j) is
// never 0 mod r)
struct g1t {
  m3xb::fp x, y;
};

// shape of a fixed-base table over 4096 points (k_kzgp_bases, k_kzgp_table)
#define KZGP_WINDOWS 64  // 4-bit windows of a 256-bit scalar
#define KZGP_DIGITS 8    // table multiples d = 1..8
#define KZGP_TABLE_POINTS ((uint64_t)KZGP_WINDOWS * 4096 * KZGP_DIGITS)

// validated setup: device-resident points of the pairing checks
struct m3x_kzg {
  int device = 0;
  m3xb::g2j *g2 = nullptr; // [0] = -[tau]G2, [1] = G2 generator (z = 1)
  // prover only (m3x_kzgp_load_g1_lagrange): the fixed-base table
  // T[j][i][d-1] = [d * 2^(4j)] L_i, affine, i in blob (bit-reversed) order
  struct g1t *table = nullptr;
  // cell verification only (m3x_kzgc_load_cell_setup)
  m3xb::g1j *cell_g1 = nullptr; // g1_monomial[0..64), z = 1
  m3xb::g2j *cell_g2 = nullptr; // [0] = -[tau^64]G2, [1] = G2 generator
  // cell proofs only (m3x_kzgc_load_g1_monomial): the same table shape over
  // g1_monomial, T[j][i][d-1] = [d * 2^(4j) tau^i]G1, i in natural order
  struct g1t *mono_table = nullptr;
};

// The helpers keep internal linkage, as they had inside m3x_kzg.hip: each
// translation unit inlines its own copy.
namespace {

__device__ __forceinline__ uint32_t ld_be32(const uint8_t *p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return __builtin_bswap32(v);
}

// Jacobian -> 48-byte compressed form, the inverse of g1_decompress: the
// sign bit follows the same lexicographic rule, infinity is 0xc0 00...
__device__ inline void g1_compress(uint8_t *out, const m3xb::g1j &p) {
  using namespace m3xb;
  if (g1j_is_inf(p)) {
    for (int i = 0; i < 48; i++) out[i] = 0;
    out[0] = 0xC0;
    return;
  }
  g1a a;
  g1j_to_aff(a, p);
  fp_to_be48(a.x, out);
  out[0] |= fp_gt_half(a.y) ? 0xA0 : 0x80;
}

// validate_kzg_g1: decompress (infinity is a valid KZG point, unlike a
// public key) + subgroup check as in k_bls_pk_decompress
__device__ inline bool kzg_validate_g1(m3xb::g1a &p, const uint8_t *src) {
  using namespace m3xb;
  return g1_decompress(p, src) == 0 && (p.inf || g1_in_subgroup(p));
}

// [k]B for an affine G1 base, 32-byte big-endian scalar, mixed adds
__device__ inline void g1_mul_be32_aff(m3xb::g1j &r, const m3xb::g1a &base,
                                       const uint8_t *be) {
  using namespace m3xb;
  g1j acc;
  g1j_set_inf(acc);
  for (int i = 0; i < 32; i++) {
    uint8_t byte = be[i];
    for (int b = 7; b >= 0; b--) {
      g1j_dbl(acc, acc);
      if ((byte >> b) & 1) g1j_add_aff(acc, acc, base);
    }
  }
  r = acc;
}

} // namespace

namespace m3x {
// k_kzg_setup: validate a compressed G2 point (decodes, in the subgroup, not
// infinity), out[0] = its negation, out[1] = the G2 generator; *fail = 0/1
void launch_kzg_setup(hipStream_t st, const uint8_t *g2_96_dev,
                      m3xb::g2j *out, int *fail);
// k_kzg_reduce_g1, both stages: *out = in[0] + ... + in[n-1]; stage holds
// 256 partial sums; skipped when *fail is set
void launch_kzg_sum_g1(hipStream_t st, const m3xb::g1j *in, uint64_t n,
                       m3xb::g1j *stage, m3xb::g1j *out, const int *fail);
// k_kzg_finish: *verdict = e(sums[0], g2[0]) * e(sums[1], g2[1]) == 1, or 0
// when *fail is set
void launch_kzg_finish(hipStream_t st, m3xb::g1j *sums, int *fail,
                       int *verdict, const m3xb::g2j *g2);
// k_kzgp_bases: validate 4096 compressed G1 points (decodes, in the subgroup,
// not infinity; *fail |= 1 otherwise), bases[j * 4096 + e] = [16^j] of entry
// bitrev12(e) of the list, j = 0..63
void launch_kzgp_bases(hipStream_t st, const uint8_t *points_dev,
                       m3xb::g1j *bases, int *fail);
// k_kzgp_table: table[(j * 4096 + e) * 8 + d - 1] = [d] bases[j * 4096 + e],
// affine
void launch_kzgp_table(hipStream_t st, const m3xb::g1j *bases, g1t *table);
} // namespace m3x
