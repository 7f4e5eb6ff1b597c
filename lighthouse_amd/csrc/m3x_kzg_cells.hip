// MI355X-native PeerDAS cell KZG (Fulu polynomial-commitments-sampling.md
// compute_cells / verify_cell_kzg_proof_batch; the seam the reference's Kzg
// wrapper stubs with TODO(das), crypto/kzg/src/lib.rs:171-216).
//
// A translation unit of its own, for the reason m3x_bls_each.hip records: a
// second caller of the shared inline helpers inside m3x_kzg.hip would change
// how that file's kernels compile. What is shared comes from m3x_kzg.hh.
//
// Conventions: omega_N = 7^((r-1)/N); cell c (0..127) holds the blob
// polynomial's values on the coset h_c * <omega_64>, h_c =
// omega_8192^bitrev7(c), element i at h_c * omega_64^bitrev6(i). Cells 0..63
// are the blob itself.
//
// fr_ntt64_wave (kzg_ntt.hh, shared with cell recovery) is the core: a
// 64-point radix-2 transform over Fr, one element per lane, the six butterfly
// stages exchanged with __shfl_xor (no LDS). The row and column steps of the
// four-step transforms come from the same header.
//
// compute_cells: each 4096-point transform is a 64 x 64 four-step
// decomposition over that core, one wave per row or column, staged through
// global scratch (2 x 128 KiB per blob, L2-resident) rather than one
// blob-sized LDS block: 64 waves per blob spread over the CUs, no
// dynamic-LDS opt-in, and no kernel holds more than one fr per lane.
//   k_kzgc_rows   decode + canonical check, copy cells 0..63, inverse rows,
//                 twiddle omega_4096^(-n2 k1) / 4096
//   k_kzgc_mid    inverse columns -> coefficients, * omega_8192^j, forward
//                 rows, twiddle omega_4096^(n2 k1)
//   k_kzgc_cols   forward columns, encode cells 64..127
//
// verify_cell_kzg_proof_batch, r = the RCKZGCBATCH__V1_ challenge:
//   before r  k_kzgc_points   validate_kzg_g1 of the m commitments, n proofs
//             k_kzgc_decode   the n*64 evaluations, canonical check
//             (host)          the transcript SHA-256, overlapping the two
//   after r   k_kzgc_powers   r^k, r^k * h_col^64
//             k_kzgc_weights  per-commitment sums of r^k
//             k_kzgc_columns  E_c = sum_{col_k = c} r^k evals_k, then one
//                             interpolation per column present
//             k_kzgc_coeffs   the 64 coefficient sums over the columns
//             k_kzgc_mults    2n + m + 64 G1 scalar multiplications
//             k_kzg_reduce_g1, k_kzg_finish (m3x_kzg.hip):
//        e(sum r^k pi_k, -[tau^64]G2) *
//        e(sum w_i C_i - sum_j a_j [tau^j]G1 + sum r^k h_col^64 pi_k, G2) == 1
#include "bls_device.hh"
#include "fr_device.hh"
#include "kzg_cell_consts.h"
#include "kzg_ntt.hh"
#include "m3x_ctx.hh"
#include "m3x_kzg.hh"
#include "../../include/m3x_consensus.h"

using namespace m3xb;
using namespace m3xf;

#define KZG_BLOB_BYTES 131072
#define KZGC_CELL 64                                  // field elements
#define KZGC_CELLS 128                                // per extended blob
#define KZGC_CELL_BYTES 2048
#define KZGC_EXT_BYTES (KZGC_CELLS * KZGC_CELL_BYTES) // one blob's cells
#define KZGC_MAX_BATCH 65535

namespace {

// ----------------------------------------------------------- compute_cells

// Inverse transform, rows. With n = 64 n1 + n2 the natural-order index of an
// evaluation, blob element 64 c + l is e[64 bitrev6(l) + bitrev6(c)]: wave
// (blob, c) reads one 64-element run of the blob, which is row n2 =
// bitrev6(c) in bit-reversed order, and is cell c as it stands.
// t1[k1 * 64 + c] = A[n2][k1] * omega_4096^(-n2 k1) / 4096.
__global__ __launch_bounds__(256) void k_kzgc_rows(
    const uint8_t *__restrict__ blobs, uint64_t n, fr *__restrict__ t1,
    uint8_t *__restrict__ cells, int *__restrict__ fail) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t c = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  const uint8_t *src = blobs + b * KZG_BLOB_BYTES + (64 * c + l) * 32;
  uint8_t *dst = cells + b * KZGC_EXT_BYTES + (64 * c + l) * 32;
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t v = ld_be32(src + 4 * i);
    s[7 - i] = v;
    st_be32(dst + 4 * i, v);
  }
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

// Wave (blob, k1): the inverse transform's column k1 gives the coefficients
// coef[k1 + 64 l] on lane l. Scaled by omega_8192^j they are the input of
// the forward transform over the odd 8192nd roots, whose row n2 = k1 they
// already form in natural order: t2[l * 64 + k1] = B[k1][bitrev6(l)] *
// omega_4096^(k1 bitrev6(l)).
__global__ __launch_bounds__(256) void k_kzgc_mid(const fr *__restrict__ t1,
                                                  uint64_t n,
                                                  fr *__restrict__ t2) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t k1 = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr a = t1[b * KZG_N + k1 * 64 + l];
  fr_ntt64_wave<false, true>(a, (int)l);
  kzgc_fwd_row<true>(a, k1, l);
  t2[b * KZG_N + l * 64 + k1] = a;
}

// Forward transform, columns. Wave (blob, c) holds column k1 = bitrev6(c) in
// natural order; lane i ends with F[bitrev6(c) + 64 bitrev6(i)] =
// F[bitrev12(64 c + i)], element i of cell 64 + c.
__global__ __launch_bounds__(256) void k_kzgc_cols(const fr *__restrict__ t2,
                                                   uint64_t n,
                                                   uint8_t *__restrict__ cells) {
  uint64_t wv = wave_index();
  uint64_t b = wv >> 6;
  uint32_t c = (uint32_t)wv & 63, l = threadIdx.x & 63;
  if (b >= n) return; // wave-uniform
  fr a = t2[b * KZG_N + c * 64 + l];
  kzgc_fwd_col_store(
      a, l, cells + b * KZGC_EXT_BYTES + (64 * (64 + c) + l) * 32);
}

struct CellsWork {
  fr *t1, *t2; // [n*4096] each
  int *fail;   // [1]
};

int cells_layout(m3x_ctx *ctx, uint64_t n, CellsWork &w) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.t1 = c.take<fr>(n * KZG_N);
        w.t2 = c.take<fr>(n * KZG_N);
        w.fail = c.take<int>(1);
      });
}

// ------------------------------------------------------------------ verify

struct CellVerifyWork {
  g1j *pts;      // [m+n] validated commitments, then proofs (z=0: infinity)
  fr *evals;     // [n*64] cell evaluations, Montgomery form
  fr *pw;        // [n] r^k
  fr *ic;        // [128*64] per-column interpolant coefficients
  uint8_t *sc;   // [(2n+m+64)*32] BE scalars, one per term (same index)
  g1j *terms;    // [2n+m+64] r^k pi_k | r^k h^64 pi_k | w_i C_i | -a_j [tau^j]G1
  g1j *stage;    // [512] stage-1 partial sums (two reductions)
  g1j *sums;     // [2] pairing arguments
  uint8_t *r;    // [32] the challenge, canonical BE
  int *fail;     // [1] encoding-error flag
  int *verdict;  // [1]
};

int cell_verify_layout(m3x_ctx *ctx, uint64_t m, uint64_t n,
                       CellVerifyWork &w) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.pts = c.take<g1j>(m + n);
        w.evals = c.take<fr>(n * KZGC_CELL);
        w.pw = c.take<fr>(n);
        w.ic = c.take<fr>(KZGC_CELLS * KZGC_CELL);
        w.sc = c.take<uint8_t>((2 * n + m + KZGC_CELL) * 32);
        w.terms = c.take<g1j>(2 * n + m + KZGC_CELL);
        w.stage = c.take<g1j>(512);
        w.sums = c.take<g1j>(2);
        w.r = c.take<uint8_t>(32);
        w.fail = c.take<int>(1);
        w.verdict = c.take<int>(1);
      });
}

// validate_kzg_g1 for the m commitments and the n proofs, one lane per point
__global__ __launch_bounds__(64, 1) void k_kzgc_points(
    const uint8_t *__restrict__ cs, uint64_t m,
    const uint8_t *__restrict__ proofs, uint64_t n, g1j *__restrict__ pts,
    int *__restrict__ fail) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= m + n) return;
  const uint8_t *src = lane < m ? cs + 48 * lane : proofs + 48 * (lane - m);
  g1a p;
  g1j out;
  if (!kzg_validate_g1(p, src)) {
    atomicOr(fail, 1);
    g1j_set_inf(out); // harmless placeholder; the call already failed
  } else {
    g1j_from_aff(out, p);
  }
  pts[lane] = out;
}

// setup validation: g1_monomial[0..64) must decode, be in the subgroup and
// not be infinity
__global__ __launch_bounds__(64, 1) void k_kzgc_setup_g1(
    const uint8_t *__restrict__ mono, g1j *__restrict__ out,
    int *__restrict__ fail) {
  uint32_t j = threadIdx.x;
  g1a p;
  if (!kzg_validate_g1(p, mono + 48 * j) || p.inf) {
    atomicOr(fail, 1);
    g1_gen(p); // placeholder; the load already failed
  }
  g1j o;
  g1j_from_aff(o, p);
  out[j] = o;
}

// the n*64 evaluations: canonical check, Montgomery form
__global__ __launch_bounds__(256) void k_kzgc_decode(
    const uint8_t *__restrict__ cells, uint64_t count, fr *__restrict__ evals,
    int *__restrict__ fail) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  fr v;
  if (!fr_from_be32(v, cells + 32 * i)) {
    atomicOr(fail, 1);
    fr_zero(v);
  }
  evals[i] = v;
}

// lane k: r^k, and the scalars of pi_k: r^k (left pairing) and
// r^k * h_col^64 = r^k * omega_128^bitrev7(col_k)
__global__ __launch_bounds__(256) void k_kzgc_powers(
    const uint64_t *__restrict__ cols, uint64_t n, CellVerifyWork w) {
  uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  fr r, p, h, w128;
  if (!fr_from_be32(r, w.r)) fr_zero(r); // the host reduces r: never taken
  fr_pow_u32(p, r, (uint32_t)k);
  w.pw[k] = p;
  fr_to_be32(p, w.sc + 32 * k);
  FRC_LOAD(w128, FRC_OMEGA8192_MONT);
  for (int i = 0; i < 6; i++) fr_sqr(w128, w128); // omega_8192^64
  fr_pow_u32(h, w128, bitrev_lo((uint32_t)cols[k], 7));
  fr_mul(h, h, p);
  fr_to_be32(h, w.sc + 32 * (n + k));
}

// lane i: the weight of commitment i, sum of r^k over the cells of row i
__global__ __launch_bounds__(256) void k_kzgc_weights(
    const uint64_t *__restrict__ rows, uint64_t n, uint64_t m,
    CellVerifyWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  fr acc;
  fr_zero(acc);
  for (uint64_t k = 0; k < n; k++)
    if (rows[k] == i) fr_add(acc, acc, w.pw[k]);
  fr_to_be32(acc, w.sc + 32 * (2 * n + i));
}

// Wave c: interpolation is linear in the evaluations of one coset, so the
// cells of column c are first combined, E_c = sum r^k evals_k, and then
// interpolated once: J = IFFT_64(E_c in natural order) / 64 and
// ic[c][j] = J[j] * h_c^(-j). A cell is its coset's values in bit-reversed
// order, the transform's input order. A column without cells stores zeros.
__global__ __launch_bounds__(64) void k_kzgc_columns(
    const uint64_t *__restrict__ cols, uint64_t n, CellVerifyWork w) {
  uint32_t c = blockIdx.x, l = threadIdx.x;
  fr acc;
  fr_zero(acc);
  bool present = false;
  for (uint64_t k = 0; k < n; k++) {
    if (cols[k] != c) continue; // wave-uniform
    fr t;
    fr_mul(t, w.pw[k], w.evals[k * KZGC_CELL + l]);
    fr_add(acc, acc, t);
    present = true;
  }
  if (present) { // wave-uniform: all 64 lanes enter the transform
    fr h, t;
    fr_ntt64_wave<false, true>(acc, (int)l);
    FRC_LOAD(h, FRC_OMEGA8192_INV_MONT);
    fr_pow_u32(t, h, bitrev_lo(c, 7) * l);
    fr_mul(acc, acc, t);
    FRC_LOAD(h, FRC_INV64_MONT);
    fr_mul(acc, acc, h);
  }
  w.ic[c * KZGC_CELL + l] = acc;
}

// lane j: a_j = sum over the columns of coefficient j; the term's scalar is
// -a_j (the interpolants are subtracted)
__global__ __launch_bounds__(64) void k_kzgc_coeffs(uint64_t n, uint64_t m,
                                                    CellVerifyWork w) {
  uint32_t j = threadIdx.x;
  fr acc;
  fr_zero(acc);
  for (int c = 0; c < KZGC_CELLS; c++) fr_add(acc, acc, w.ic[c * KZGC_CELL + j]);
  fr_neg(acc, acc);
  fr_to_be32(acc, w.sc + 32 * (2 * n + m + j));
}

// the 2n + m + 64 independent scalar multiplications, one lane each
// (k_kzg_mults' shape); term i takes scalar i
__global__ __launch_bounds__(64, 1) void k_kzgc_mults(
    uint64_t n, uint64_t m, const g1j *__restrict__ cell_g1,
    CellVerifyWork w) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * n + m + KZGC_CELL) return;
  if (*w.fail) return;
  const g1j *src;
  if (lane < n)
    src = &w.pts[m + lane];
  else if (lane < 2 * n)
    src = &w.pts[m + (lane - n)];
  else if (lane < 2 * n + m)
    src = &w.pts[lane - 2 * n];
  else
    src = &cell_g1[lane - 2 * n - m];
  g1a base;
  base.inf = g1j_is_inf(*src) ? 1 : 0;
  base.x = src->x; // z == 1: affine coordinates
  base.y = src->y;
  g1j out;
  if (base.inf)
    g1j_set_inf(out);
  else
    g1_mul_be32_aff(out, base, w.sc + 32 * lane);
  w.terms[lane] = out;
}

// ------------------------------------------------------- host: transcript

// SHA-256 (FIPS 180-4) of the transcript, on the calling thread: one message
// is serial, and here it overlaps the device's point validation.
struct HostSha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint8_t buf[64];
  uint64_t len = 0;

  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

  void block(const uint8_t *p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu,
        0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u,
        0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u,
        0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
        0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u,
        0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
      w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) |
             ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5],
             g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
      uint32_t t1 = hh + S1 + ((e & f) ^ (~e & g)) + K[i] + w[i];
      uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
      uint32_t t2 = S0 + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
    h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }

  void update(const uint8_t *p, uint64_t n) {
    uint32_t fill = (uint32_t)(len & 63);
    len += n;
    if (fill) {
      uint32_t take = 64 - fill;
      if (take > n) take = (uint32_t)n;
      for (uint32_t i = 0; i < take; i++) buf[fill + i] = p[i];
      p += take;
      n -= take;
      if (fill + take < 64) return;
      block(buf);
    }
    for (; n >= 64; p += 64, n -= 64) block(p);
    for (uint64_t i = 0; i < n; i++) buf[i] = p[i];
  }

  void be64(uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * (7 - i)));
    update(b, 8);
  }

  void finish(uint8_t out[32]) {
    uint64_t bits = len * 8;
    uint8_t pad[72] = {0x80};
    uint32_t fill = (uint32_t)(len & 63);
    uint32_t padlen = fill < 56 ? 56 - fill : 120 - fill;
    update(pad, padlen);
    be64(bits);
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(h[i] >> 24);
      out[4 * i + 1] = (uint8_t)(h[i] >> 16);
      out[4 * i + 2] = (uint8_t)(h[i] >> 8);
      out[4 * i + 3] = (uint8_t)h[i];
    }
  }
};

// hash_to_bls_field of "RCKZGCBATCH__V1_" | BE64(4096) | BE64(64) | BE64(m) |
// BE64(n) | commitments | per cell: BE64(row) BE64(col) cell proof
void cell_batch_challenge(const uint8_t *cs, uint64_t m, const uint64_t *rows,
                          const uint64_t *cols, const uint8_t *cells,
                          const uint8_t *proofs, uint64_t n,
                          uint8_t out_r[32]) {
  static const uint8_t domain[16] = {'R', 'C', 'K', 'Z', 'G', 'C', 'B', 'A',
                                     'T', 'C', 'H', '_', '_', 'V', '1', '_'};
  HostSha256 s;
  s.update(domain, 16);
  s.be64(KZG_N);
  s.be64(KZGC_CELL);
  s.be64(m);
  s.be64(n);
  s.update(cs, 48 * m);
  for (uint64_t k = 0; k < n; k++) {
    s.be64(rows[k]);
    s.be64(cols[k]);
    s.update(cells + KZGC_CELL_BYTES * k, KZGC_CELL_BYTES);
    s.update(proofs + 48 * k, 48);
  }
  uint8_t dg[32];
  s.finish(dg);
  // mod r: 2^256 < 3r, so at most two subtractions
  uint32_t v[8];
  for (int i = 0; i < 8; i++)
    v[7 - i] = ((uint32_t)dg[4 * i] << 24) | ((uint32_t)dg[4 * i + 1] << 16) |
               ((uint32_t)dg[4 * i + 2] << 8) | dg[4 * i + 3];
  for (int pass = 0; pass < 2; pass++) {
    bool ge = true;
    for (int i = 7; i >= 0; i--) {
      if (v[i] > FR_MOD[i]) break;
      if (v[i] < FR_MOD[i]) {
        ge = false;
        break;
      }
    }
    if (!ge) break;
    uint64_t bw = 0;
    for (int i = 0; i < 8; i++) {
      uint64_t x = (uint64_t)v[i] - FR_MOD[i] - bw;
      v[i] = (uint32_t)x;
      bw = (x >> 32) & 1;
    }
  }
  for (int i = 0; i < 8; i++) {
    out_r[4 * i] = (uint8_t)(v[7 - i] >> 24);
    out_r[4 * i + 1] = (uint8_t)(v[7 - i] >> 16);
    out_r[4 * i + 2] = (uint8_t)(v[7 - i] >> 8);
    out_r[4 * i + 3] = (uint8_t)v[7 - i];
  }
}

// the checks made before anything is launched
bool cell_batch_args_ok(const uint8_t *cs, uint64_t m, const uint64_t *rows,
                        const uint64_t *cols, const uint8_t *cells,
                        const uint8_t *proofs, uint64_t n) {
  if (m == 0 || !cs || !rows || !cols || !cells || !proofs) return false;
  for (uint64_t k = 0; k < n; k++)
    if (rows[k] >= m || cols[k] >= KZGC_CELLS) return false;
  return true;
}

uint32_t blocks_of(uint64_t lanes, uint32_t per) {
  return (uint32_t)((lanes + per - 1) / per);
}

} // namespace

extern "C" {

int32_t m3x_kzgc_compute_cells_dev(m3x_ctx *ctx, const void *blobs_dev,
                                  uint64_t n, void *cells_out_dev) {
  if (!ctx || n > KZGC_MAX_BATCH) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs_dev || !cells_out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  CellsWork w;
  int rc = cells_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  // 64 waves per blob and pass, 4 waves per block: every wave is full
  dim3 grid((uint32_t)(n * 16)), block(256);
  m3x::time_begin(ctx, M3X_K_KZGC_NTT);
  hipLaunchKernelGGL(k_kzgc_rows, grid, block, 0, ctx->stream,
                     (const uint8_t *)blobs_dev, n, w.t1,
                     (uint8_t *)cells_out_dev, w.fail);
  hipLaunchKernelGGL(k_kzgc_mid, grid, block, 0, ctx->stream, w.t1, n, w.t2);
  hipLaunchKernelGGL(k_kzgc_cols, grid, block, 0, ctx->stream, w.t2, n,
                     (uint8_t *)cells_out_dev);
  m3x::time_end(ctx, M3X_K_KZGC_NTT);
  int32_t fail = 1;
  M3X_HIP_CHECK(
      hipMemcpyAsync(&fail, w.fail, 4, hipMemcpyDeviceToHost, ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

int32_t m3x_kzgc_compute_cells(m3x_ctx *ctx, const uint8_t *blobs, uint64_t n,
                              uint8_t *cells_out) {
  if (!ctx || n > KZGC_MAX_BATCH) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs || !cells_out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES);
  uint8_t *out_d = tmp.alloc(n * KZGC_EXT_BYTES);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t rc = m3x_kzgc_compute_cells_dev(ctx, bl_d, n, out_d);
  if (rc != M3X_OK) return rc;
  tmp.download(cells_out, out_d, n * KZGC_EXT_BYTES);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_kzgc_load_cell_setup(m3x_ctx *ctx, m3x_kzg *kzg,
                                const uint8_t *g1_monomial64,
                                const uint8_t g2_tau64[96]) {
  if (!ctx || !kzg || !kzg->g2 || kzg->device != ctx->device ||
      !g1_monomial64 || !g2_tau64 || kzg->cell_g1)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *g1_d = tmp.upload(g1_monomial64, (uint64_t)KZGC_CELL * 48);
  const uint8_t *g2_d = tmp.upload(g2_tau64, 96);
  g1j *g1 = tmp.alloc<g1j>(KZGC_CELL * sizeof(g1j));
  g2j *g2 = tmp.alloc<g2j>(2 * sizeof(g2j));
  int *fail_d = tmp.alloc<int>(8);
  if (!tmp.ok()) return M3X_ERR_HIP;
  M3X_HIP_CHECK(hipMemsetAsync(fail_d, 0, 8, ctx->stream));
  hipLaunchKernelGGL(k_kzgc_setup_g1, dim3(1), dim3(KZGC_CELL), 0, ctx->stream,
                     g1_d, g1, fail_d);
  m3x::launch_kzg_setup(ctx->stream, g2_d, g2, fail_d + 1);
  int fail[2] = {1, 1};
  tmp.download(fail, fail_d, 8);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail[0] || fail[1]) return M3X_ERR_ENCODING;
  kzg->cell_g1 = tmp.release(g1); // the handle owns both from here
  kzg->cell_g2 = tmp.release(g2);
  return M3X_OK;
}

int32_t m3x_kzgc_verify_cell_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const uint8_t *commitments, uint64_t m,
                                        const uint64_t *rows,
                                        const uint64_t *cols,
                                        const uint8_t *cells,
                                        const uint8_t *proofs, uint64_t n) {
  if (!ctx || !kzg || !kzg->cell_g1 || !kzg->cell_g2 ||
      kzg->device != ctx->device || n > KZGC_MAX_BATCH)
    return M3X_ERR_ARG;
  if (n == 0) return 1;
  if (!cell_batch_args_ok(commitments, m, rows, cols, cells, proofs, n))
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  CellVerifyWork w;
  int rc = cell_verify_layout(ctx, m, n, w);
  if (rc != M3X_OK) return rc;
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *cs_d = tmp.upload(commitments, m * 48),
                *pr_d = tmp.upload(proofs, n * 48),
                *ce_d = tmp.upload(cells, n * KZGC_CELL_BYTES);
  const uint64_t *rows_d = tmp.upload(rows, n * 8),
                 *cols_d = tmp.upload(cols, n * 8);
  if (!tmp.ok()) return M3X_ERR_HIP;
  hipStream_t st = ctx->stream;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, st));
  // before r: everything that needs no challenge
  m3x::time_begin(ctx, M3X_K_KZG_DECOMP);
  hipLaunchKernelGGL(k_kzgc_points, dim3(blocks_of(m + n, 64)), dim3(64), 0, st,
                     cs_d, m, pr_d, n, w.pts, w.fail);
  m3x::time_end(ctx, M3X_K_KZG_DECOMP);
  m3x::time_begin(ctx, M3X_K_KZGC_DECODE);
  hipLaunchKernelGGL(k_kzgc_decode, dim3(blocks_of(n * KZGC_CELL, 256)),
                     dim3(256), 0, st, ce_d, n * KZGC_CELL, w.evals, w.fail);
  m3x::time_end(ctx, M3X_K_KZGC_DECODE);
  // the transcript hash runs here while the device validates the points
  uint8_t r[32];
  cell_batch_challenge(commitments, m, rows, cols, cells, proofs, n, r);
  M3X_HIP_CHECK(hipMemcpyAsync(w.r, r, 32, hipMemcpyHostToDevice, st));
  // after r
  m3x::time_begin(ctx, M3X_K_KZGC_COMBINE);
  hipLaunchKernelGGL(k_kzgc_powers, dim3(blocks_of(n, 256)), dim3(256), 0, st,
                     cols_d, n, w);
  hipLaunchKernelGGL(k_kzgc_weights, dim3(blocks_of(m, 256)), dim3(256), 0, st,
                     rows_d, n, m, w);
  hipLaunchKernelGGL(k_kzgc_columns, dim3(KZGC_CELLS), dim3(64), 0, st, cols_d,
                     n, w);
  hipLaunchKernelGGL(k_kzgc_coeffs, dim3(1), dim3(KZGC_CELL), 0, st, n, m, w);
  m3x::time_end(ctx, M3X_K_KZGC_COMBINE);
  m3x::time_begin(ctx, M3X_K_KZG_MULTS);
  hipLaunchKernelGGL(k_kzgc_mults,
                     dim3(blocks_of(2 * n + m + KZGC_CELL, 64)), dim3(64), 0,
                     st, n, m, kzg->cell_g1, w);
  m3x::time_end(ctx, M3X_K_KZG_MULTS);
  m3x::time_begin(ctx, M3X_K_KZG_REDUCE);
  m3x::launch_kzg_sum_g1(st, w.terms, n, w.stage, w.sums, w.fail);
  m3x::launch_kzg_sum_g1(st, w.terms + n, n + m + KZGC_CELL, w.stage + 256,
                         w.sums + 1, w.fail);
  m3x::time_end(ctx, M3X_K_KZG_REDUCE);
  m3x::time_begin(ctx, M3X_K_KZG_FINISH);
  m3x::launch_kzg_finish(st, w.sums, w.fail, w.verdict, kzg->cell_g2);
  m3x::time_end(ctx, M3X_K_KZG_FINISH);
  int32_t verdict = 0, fail = 1;
  tmp.download(&verdict, w.verdict, 4);
  tmp.download(&fail, w.fail, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail) return M3X_ERR_ENCODING;
  return verdict;
}

int32_t m3x_kzgc_cell_batch_challenge_test(m3x_ctx *ctx,
                                          const uint8_t *commitments,
                                          uint64_t m, const uint64_t *rows,
                                          const uint64_t *cols,
                                          const uint8_t *cells,
                                          const uint8_t *proofs, uint64_t n,
                                          uint8_t out_r[32]) {
  if (!ctx || !out_r || n == 0 || n > KZGC_MAX_BATCH ||
      !cell_batch_args_ok(commitments, m, rows, cols, cells, proofs, n))
    return M3X_ERR_ARG;
  cell_batch_challenge(commitments, m, rows, cols, cells, proofs, n, out_r);
  return M3X_OK;
}

} // extern "C"
