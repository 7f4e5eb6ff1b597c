// MI355X-native KZG blob proof verification (Deneb polynomial-commitments.md
// verify_kzg_proof / verify_blob_kzg_proof / verify_blob_kzg_proof_batch;
// the reference's crypto/kzg/src/lib.rs:83-167 surface).
//
// Pipeline for n (blob, commitment, proof) triples, big-endian everywhere:
//   k_kzg_challenge  z_i = SHA256(domain | degree | blob_i | C_i) mod r —
//                    one lane per blob, on stream2
//   k_kzg_decomp     decompress + subgroup-check every C_i and pi_i (2n
//                    lanes); independent of z, so it overlaps the hash
//   k_kzg_eval       y_i = p_i(z_i), barycentric over the bit-reversed
//                    4096th roots of unity, one 256-thread block per blob
//   k_kzg_batch_r    r = SHA256(domain | 4096 | n | C_i z_i y_i pi_i ...)
//                    mod r and the scalars r^i, r^i z_i, -sum r^i y_i
//   k_kzg_mults      the 3n+1 independent 255-bit G1 scalar mults, one
//                    lane each
//   k_kzg_reduce_g1  two-stage Jacobian sums (k_bls_reduce_sig's shape)
//   k_kzg_finish     one wave:
//        e(sum r^i pi_i, -[tau]G2) *
//        e(sum r^i (C_i - y_i G1) + sum r^i z_i pi_i, G2) == 1
// The batch equation is used for n == 1 too (r^0 = 1): it is algebraically
// the spec's single-proof check and needs no G2 scalar multiplication.
// Integer VALU workload (no MFMA); Fp/G1/pairing code is bls_device.hh's.
//
// The producing half (blob_to_kzg_commitment, compute_kzg_proof,
// compute_blob_kzg_proof; lib.rs:72-81, 134-150) is the "prover" section
// further down: a fixed-base G1 MSM over the Lagrange setup points.
#include "bls_device.hh"
#include "fr_device.hh"
#include "m3x_ctx.hh"
#include "m3x_kzg.hh"
#include "../../include/m3x_consensus.h"

using namespace m3xb;
using namespace m3xf;

#define KZG_N 4096
#define KZG_BLOB_BYTES 131072
#define KZG_MAX_BATCH 65535 // one grid dimension; far above any block's blobs

namespace {

struct KzgWork {
  uint8_t *zs;     // [n*32] challenges, canonical BE
  uint8_t *ys;     // [n*32] evaluations, canonical BE
  uint8_t *tr;     // [32+160n] batch-challenge transcript
  uint8_t *sc;     // [(2n+1)*32] BE scalars: r^i | r^i z_i | -sum r^i y_i
  uint8_t *r_out;  // [32] the batch challenge
  g1j *pts;        // [2n] validated commitments, then proofs (z=0: infinity)
  g1j *terms;      // [3n+1] r^i pi_i | r^i z_i pi_i | r^i C_i | -(sum r^i y_i)G1
  g1j *stage;      // [512] stage-1 partial sums (two reductions)
  g1j *sums;       // [2] pairing arguments
  int *fail;       // [1] encoding-error flag
  int *verdict;    // [1]
};

// "FSBLOBVERIFY_V1_" / "RCKZGBATCH___V1_" as big-endian words / bytes
__device__ __constant__ static const uint32_t KZG_FS_DOMAIN[4] = {
    0x4653424cu, 0x4f425645u, 0x52494659u, 0x5f56315fu};
__device__ __constant__ static const uint8_t KZG_RC_DOMAIN[16] = {
    'R', 'C', 'K', 'Z', 'G', 'B', 'A', 'T', 'C', 'H', '_', '_', '_', 'V', '1', '_'};

// ---------------------------------------------------------------- kernels

// compute_challenge: the 131152-byte message is 2050 compressions; block 0
// is domain | BE128(4096) | blob[0:32], so every later block reads the
// blob at a 32-byte offset. SHA-256 of one message is serial: one lane.
__global__ __launch_bounds__(64) void k_kzg_challenge(
    const uint8_t *__restrict__ blobs, const uint8_t *__restrict__ cs,
    uint64_t n, KzgWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *blob = blobs + i * KZG_BLOB_BYTES;
  const uint8_t *c = cs + 48 * i;
  m3x::Sha256State s;
  m3x::sha256_init(s);
  uint32_t m[16];
#pragma unroll
  for (int k = 0; k < 4; k++) m[k] = KZG_FS_DOMAIN[k];
  m[4] = 0;
  m[5] = 0;
  m[6] = 0;
  m[7] = KZG_N;
#pragma unroll
  for (int k = 0; k < 8; k++) m[8 + k] = ld_be32(blob + 4 * k);
  m3x::sha256_compress(s, m);
  for (uint32_t b = 1; b < 2048; b++) {
    const uint8_t *p = blob + 64 * b - 32;
#pragma unroll
    for (int k = 0; k < 16; k++) m[k] = ld_be32(p + 4 * k);
    m3x::sha256_compress(s, m);
  }
#pragma unroll
  for (int k = 0; k < 8; k++)
    m[k] = ld_be32(blob + KZG_BLOB_BYTES - 32 + 4 * k);
#pragma unroll
  for (int k = 0; k < 8; k++) m[8 + k] = ld_be32(c + 4 * k);
  m3x::sha256_compress(s, m);
#pragma unroll
  for (int k = 0; k < 4; k++) m[k] = ld_be32(c + 32 + 4 * k);
  m[4] = 0x80000000u;
#pragma unroll
  for (int k = 5; k < 15; k++) m[k] = 0;
  m[15] = (32 + KZG_BLOB_BYTES + 48) * 8;
  m3x::sha256_compress(s, m);
  uint8_t dg[32];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    dg[4 * k] = (uint8_t)(s.h[k] >> 24);
    dg[4 * k + 1] = (uint8_t)(s.h[k] >> 16);
    dg[4 * k + 2] = (uint8_t)(s.h[k] >> 8);
    dg[4 * k + 3] = (uint8_t)s.h[k];
  }
  fr z;
  fr_from_be32_reduce(z, dg);
  fr_to_be32(z, w.zs + 32 * i);
}

__device__ __forceinline__ uint32_t bitrev_lo(uint32_t v, int bits) {
  return __builtin_bitreverse32(v) >> (32 - bits);
}

// A thread's walk over the evaluation domain: of a blob's 256 threads,
// thread t owns elements 16t..16t+15. bitrev12(16t+k) = bitrev4(k)<<8 |
// bitrev8(t), so the thread's roots are omega^bitrev8(t) *
// (omega^256)^bitrev4(k): one 8-bit power and 15 multiplies, no table.
// Step mi visits k = bitrev4(mi), which makes the second factor
// (omega^256)^mi, one multiply per step.
struct DomainWalk {
  fr w16, base, g;
  uint32_t first;
  __device__ __forceinline__ void init(int t) {
    fr omega;
#pragma unroll
    for (int i = 0; i < 8; i++) omega.v[i] = FR_OMEGA_MONT[i];
    w16 = omega;
    for (int i = 0; i < 8; i++) fr_sqr(w16, w16); // omega^256
    uint32_t e = bitrev_lo((uint32_t)t, 8);
    fr_pow(base, omega, &e, 1);
    fr_one(g);
    first = 16u * (uint32_t)t;
  }
  // the element step mi visits
  __device__ __forceinline__ uint32_t index(int mi) const {
    return first + bitrev_lo((uint32_t)mi, 4);
  }
  // steps mi = 0..15 in order: the element j and wk = omega^bitrev12(j)
  __device__ __forceinline__ uint32_t next(int mi, fr &wk) {
    fr_mul(wk, base, g);
    fr_mul(g, g, w16);
    return index(mi);
  }
};

// Montgomery's trick for a thread's 16 denominators: push() them in order,
// one Fermat inversion, then pop() hands the inverses back last to first.
// The running product is the caller's local: as a member it would stay in
// scratch memory with the arrays (32 B more per lane, measurably slower).
struct BatchInv16 {
  fr den[16], pre[16];
  __device__ __forceinline__ void init(fr &run) { fr_one(run); }
  __device__ __forceinline__ void push(fr &run, int mi, const fr &d) {
    den[mi] = d;
    fr_mul(run, run, d);
    pre[mi] = run;
  }
  __device__ __forceinline__ void invert(fr &run) { fr_inv(run, run); }
  // id = 1/den[mi]; call for mi = 15 down to 0
  __device__ __forceinline__ void pop(fr &run, int mi, fr &id) {
    if (mi > 0)
      fr_mul(id, run, pre[mi - 1]);
    else
      id = run;
    fr_mul(run, run, den[mi]);
  }
};

struct fr_add_op {
  __device__ __forceinline__ void operator()(fr &r, const fr &a,
                                             const fr &b) const {
    fr_add(r, a, b);
  }
};

// evaluate_polynomial_in_evaluation_form: one block per blob, 16 elements
// per thread; the 16 denominators z - omega_j share one inversion.
__global__ __launch_bounds__(256) void k_kzg_eval(
    const uint8_t *__restrict__ blobs, uint64_t n, KzgWork w) {
  __shared__ fr lds[256];
  __shared__ fr s_hitval;
  __shared__ int s_hit;
  uint64_t b = blockIdx.x;
  int t = threadIdx.x;
  if (b >= n) return;
  const uint8_t *blob = blobs + b * KZG_BLOB_BYTES;
  if (t == 0) s_hit = 0;
  __syncthreads();
  fr z;
  if (!fr_from_be32(z, w.zs + 32 * b)) { // block-uniform
    if (t == 0) atomicOr(w.fail, 1);
    return;
  }
  DomainWalk dw;
  BatchInv16 bi;
  dw.init(t);
  fr run;
  bi.init(run);
  fr num[16];
  bool bad = false;
  for (int mi = 0; mi < 16; mi++) {
    fr f, wk, d;
    uint32_t j = dw.next(mi, wk);
    if (!fr_from_be32(f, blob + 32 * j)) {
      bad = true;
      fr_zero(f);
    }
    fr_sub(d, z, wk);
    if (fr_is_zero(d)) { // z is in the domain: y = f_j, no division
      s_hitval = f;
      s_hit = 1;
      fr_one(d);
    }
    fr_mul(num[mi], f, wk);
    bi.push(run, mi, d);
  }
  if (bad) atomicOr(w.fail, 1);
  fr acc;
  bi.invert(run);
  fr_zero(acc);
  for (int mi = 15; mi >= 0; mi--) {
    fr id, term;
    bi.pop(run, mi, id);
    fr_mul(term, num[mi], id);
    fr_add(acc, acc, term);
  }
  lds[t] = acc;
  block_tree_reduce<fr, 256>(lds, t, fr_add_op{});
  if (t == 0) {
    fr y;
    if (s_hit) {
      y = s_hitval;
    } else {
      fr zn, one, ninv;
      zn = z;
      for (int i = 0; i < 12; i++) fr_sqr(zn, zn); // z^4096
      fr_one(one);
      fr_sub(zn, zn, one);
#pragma unroll
      for (int i = 0; i < 8; i++) ninv.v[i] = FR_N_INV_MONT[i];
      fr_mul(y, lds[0], zn);
      fr_mul(y, y, ninv);
    }
    fr_to_be32(y, w.ys + 32 * b);
  }
}

// verify_kzg_proof_batch's challenge and its powers. The block assembles
// the transcript in parallel; lane 0 hashes it and walks the powers.
__global__ __launch_bounds__(256) void k_kzg_batch_r(
    const uint8_t *__restrict__ cs, const uint8_t *__restrict__ proofs,
    uint64_t n, KzgWork w) {
  uint32_t len = 32 + 160 * (uint32_t)n;
  for (uint32_t idx = threadIdx.x; idx < len; idx += blockDim.x) {
    uint8_t v;
    if (idx < 16) {
      v = KZG_RC_DOMAIN[idx];
    } else if (idx < 24) {
      v = (uint8_t)((uint64_t)KZG_N >> (8 * (23 - idx)));
    } else if (idx < 32) {
      v = (uint8_t)(n >> (8 * (31 - idx)));
    } else {
      uint32_t q = (idx - 32) / 160, o = (idx - 32) % 160;
      if (o < 48)
        v = cs[48 * q + o];
      else if (o < 80)
        v = w.zs[32 * q + (o - 48)];
      else if (o < 112)
        v = w.ys[32 * q + (o - 80)];
      else
        v = proofs[48 * q + (o - 112)];
    }
    w.tr[idx] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint8_t dg[32];
  m3x::sha256_bytes(w.tr, len, dg);
  fr rr, pw, sy;
  fr_from_be32_reduce(rr, dg);
  fr_to_be32(rr, w.r_out);
  fr_one(pw);
  fr_zero(sy);
  bool bad = false;
  for (uint64_t i = 0; i < n; i++) {
    fr z, y, t;
    if (!fr_from_be32(z, w.zs + 32 * i) || !fr_from_be32(y, w.ys + 32 * i)) {
      bad = true; // out-of-range z or y
      fr_zero(z);
      fr_zero(y);
    }
    fr_to_be32(pw, w.sc + 32 * i);
    fr_mul(t, pw, z);
    fr_to_be32(t, w.sc + 32 * (n + i));
    fr_mul(t, pw, y);
    fr_add(sy, sy, t);
    fr_mul(pw, pw, rr);
  }
  fr_neg(sy, sy);
  fr_to_be32(sy, w.sc + 32 * (2 * n));
  if (bad) atomicOr(w.fail, 1);
}

// validate_kzg_g1 for every commitment and proof. One lane per point.
__global__ __launch_bounds__(64, 1) void k_kzg_decomp(
    const uint8_t *__restrict__ cs, const uint8_t *__restrict__ proofs,
    uint64_t n, KzgWork w) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * n) return;
  const uint8_t *src = lane < n ? cs + 48 * lane : proofs + 48 * (lane - n);
  g1a p;
  bool ok = kzg_validate_g1(p, src);
  g1j out;
  if (!ok) {
    atomicOr(w.fail, 1);
    g1j_set_inf(out); // harmless placeholder; the call already failed
  } else {
    g1j_from_aff(out, p);
  }
  w.pts[lane] = out;
}

// the 3n+1 independent scalar multiplications, one lane each, four
// role-contiguous classes: r^i pi_i | (r^i z_i) pi_i | r^i C_i | the
// single folded -(sum r^i y_i) G1. At 1-6 blobs the serial 255-bit chain
// is the latency, so no lane carries more than one chain.
__global__ __launch_bounds__(64, 1) void k_kzg_mults(uint64_t n, KzgWork w) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane > 3 * n) return;
  if (*w.fail) return;
  g1a base;
  const uint8_t *k;
  if (lane == 3 * n) {
    g1_gen(base);
    k = w.sc + 32 * (2 * n);
  } else {
    uint64_t cls = lane / n, i = lane % n;
    const g1j &src = cls == 2 ? w.pts[i] : w.pts[n + i];
    base.inf = g1j_is_inf(src) ? 1 : 0;
    base.x = src.x; // z == 1: affine coordinates
    base.y = src.y;
    k = w.sc + 32 * (cls == 1 ? n + i : i);
  }
  g1j out;
  if (base.inf)
    g1j_set_inf(out);
  else
    g1_mul_be32_aff(out, base, k);
  w.terms[lane] = out;
}

// two-stage Jacobian G1 sum (block_span_reduce, as k_bls_reduce_sig); a
// failed call skips the work
__global__ __launch_bounds__(256) void k_kzg_reduce_g1(
    const g1j *__restrict__ in, uint64_t n, g1j *__restrict__ out,
    const int *__restrict__ fail) {
  __shared__ g1j lds[256];
  if (*fail) return;
  block_span_reduce<g1j, 256>(in, n, out, lds, g1j_add_op{},
                              [](g1j &r) { g1j_set_inf(r); });
}

// the pairing check, one wave (k_bls_finish's shape). miller_w returns one
// for an infinity argument, which covers all-infinity batches.
__global__ __launch_bounds__(64) void k_kzg_finish(KzgWork w,
                                                   const g2j *__restrict__ g2) {
  __shared__ fp12m sh[7];
  __shared__ f12w_ws ws;
  __shared__ miller_ws mws;
  int lane = threadIdx.x;
  if (*w.fail) {
    if (lane == 0) *w.verdict = 0;
    return;
  }
  miller_w(sh[0], w.sums[0], g2[0], ws, mws, lane);
  f12w_sync();
  miller_w(sh[1], w.sums[1], g2[1], ws, mws, lane);
  f12w_sync();
  f12_mul_w(sh[1], sh[0], sh[1], ws, lane);
  final_exp_w(sh[2], sh[1], &sh[3], ws, lane);
  if (lane == 0) *w.verdict = f12_is_one(sh[2]) ? 1 : 0;
}

// setup validation: [tau]G2 must decode, be in the subgroup, not infinity
__global__ void k_kzg_setup(const uint8_t *__restrict__ tau96,
                            g2j *__restrict__ out, int *__restrict__ fail) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  g2a t;
  if (g2_decompress(t, tau96) != 0 || t.inf || !g2_in_subgroup(t)) {
    *fail = 1;
    return;
  }
  *fail = 0;
  out[0].x = t.x;
  fp2_neg(out[0].y, t.y);
  fp2_one(out[0].z);
  FP_LOAD_C(out[1].x.c0, BLS_G2X_C0);
  FP_LOAD_C(out[1].x.c1, BLS_G2X_C1);
  FP_LOAD_C(out[1].y.c0, BLS_G2Y_C0);
  FP_LOAD_C(out[1].y.c1, BLS_G2Y_C1);
  fp2_one(out[1].z);
}

// ------------------------------------------------------------------- host

int kzg_layout(m3x_ctx *ctx, uint64_t n, KzgWork &w) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.zs = c.take<uint8_t>(n * 32);
        w.ys = c.take<uint8_t>(n * 32);
        w.tr = c.take<uint8_t>(32 + 160 * n);
        w.sc = c.take<uint8_t>((2 * n + 1) * 32);
        w.r_out = c.take<uint8_t>(32);
        w.pts = c.take<g1j>(2 * n);
        w.terms = c.take<g1j>(3 * n + 1);
        w.stage = c.take<g1j>(512);
        w.sums = c.take<g1j>(2);
        w.fail = c.take<int>(1);
        w.verdict = c.take<int>(1);
      });
}

// the per-blob challenge hash, on stream2; ev_s2 marks its end
int launch_challenge(m3x_ctx *ctx, const KzgWork &w, const uint8_t *blobs_dev,
                     const uint8_t *cs_dev, uint64_t n) {
  m3x::time_begin_s(ctx, M3X_K_KZG_CHALLENGE, ctx->stream2);
  hipLaunchKernelGGL(k_kzg_challenge, dim3((uint32_t)((n + 63) / 64)),
                     dim3(64), 0, ctx->stream2, blobs_dev, cs_dev, n, w);
  m3x::time_end_s(ctx, M3X_K_KZG_CHALLENGE, ctx->stream2);
  M3X_HIP_CHECK(hipEventRecord(ctx->ev_s2, ctx->stream2));
  return M3X_OK;
}

// the evaluation, on the main stream; hashed = true waits for the challenge
int launch_eval(m3x_ctx *ctx, const KzgWork &w, const uint8_t *blobs_dev,
                uint64_t n, bool hashed) {
  if (hashed) M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_s2, 0));
  m3x::time_begin(ctx, M3X_K_KZG_EVAL);
  hipLaunchKernelGGL(k_kzg_eval, dim3((uint32_t)n), dim3(256), 0, ctx->stream,
                     blobs_dev, n, w);
  m3x::time_end(ctx, M3X_K_KZG_EVAL);
  return M3X_OK;
}

// challenge + evaluation; zs_dev != nullptr supplies explicit z
int launch_challenge_eval(m3x_ctx *ctx, const KzgWork &w,
                          const uint8_t *blobs_dev, const uint8_t *cs_dev,
                          const uint8_t *zs_dev, uint64_t n) {
  if (zs_dev)
    M3X_HIP_CHECK(hipMemcpyAsync(w.zs, zs_dev, n * 32,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  else if (int rc = launch_challenge(ctx, w, blobs_dev, cs_dev, n))
    return rc;
  return launch_eval(ctx, w, blobs_dev, n, !zs_dev);
}

// blobs_dev != nullptr: blob batch (z, y computed on the device);
// otherwise zs_dev/ys_dev hold the caller's z and y
int run_kzg(m3x_ctx *ctx, m3x_kzg *kzg, const uint8_t *blobs_dev,
            const uint8_t *cs_dev, const uint8_t *zs_dev,
            const uint8_t *ys_dev, const uint8_t *proofs_dev, uint64_t n,
            int32_t *out) {
  KzgWork w;
  int rc = kzg_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  uint32_t blocks2 = (uint32_t)((2 * n + 63) / 64);
  // point validation does not depend on z: it runs on the main stream
  // while the serial challenge hash runs on stream2
  if (blobs_dev) {
    rc = launch_challenge(ctx, w, blobs_dev, cs_dev, n);
    if (rc != M3X_OK) return rc;
  } else {
    M3X_HIP_CHECK(hipMemcpyAsync(w.zs, zs_dev, n * 32,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    M3X_HIP_CHECK(hipMemcpyAsync(w.ys, ys_dev, n * 32,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  }
  m3x::time_begin(ctx, M3X_K_KZG_DECOMP);
  hipLaunchKernelGGL(k_kzg_decomp, dim3(blocks2), dim3(64), 0, ctx->stream,
                     cs_dev, proofs_dev, n, w);
  m3x::time_end(ctx, M3X_K_KZG_DECOMP);
  if (blobs_dev) {
    rc = launch_eval(ctx, w, blobs_dev, n, true);
    if (rc != M3X_OK) return rc;
  }
  m3x::time_begin(ctx, M3X_K_KZG_BATCH_R);
  hipLaunchKernelGGL(k_kzg_batch_r, dim3(1), dim3(256), 0, ctx->stream,
                     cs_dev, proofs_dev, n, w);
  m3x::time_end(ctx, M3X_K_KZG_BATCH_R);
  m3x::time_begin(ctx, M3X_K_KZG_MULTS);
  hipLaunchKernelGGL(k_kzg_mults, dim3((uint32_t)((3 * n + 1 + 63) / 64)),
                     dim3(64), 0, ctx->stream, n, w);
  m3x::time_end(ctx, M3X_K_KZG_MULTS);
  m3x::time_begin(ctx, M3X_K_KZG_REDUCE);
  {
    uint64_t na = n, nb = 2 * n + 1;
    uint32_t ra = (uint32_t)((na + 255) / 256), rb = (uint32_t)((nb + 255) / 256);
    if (ra > 256) ra = 256;
    if (rb > 256) rb = 256;
    hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(ra), dim3(256), 0, ctx->stream,
                       w.terms, na, w.stage, w.fail);
    hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(1), dim3(256), 0, ctx->stream,
                       w.stage, (uint64_t)ra, w.sums, w.fail);
    hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(rb), dim3(256), 0, ctx->stream,
                       w.terms + n, nb, w.stage + 256, w.fail);
    hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(1), dim3(256), 0, ctx->stream,
                       w.stage + 256, (uint64_t)rb, w.sums + 1, w.fail);
  }
  m3x::time_end(ctx, M3X_K_KZG_REDUCE);
  m3x::time_begin(ctx, M3X_K_KZG_FINISH);
  hipLaunchKernelGGL(k_kzg_finish, dim3(1), dim3(64), 0, ctx->stream, w,
                     kzg->g2);
  m3x::time_end(ctx, M3X_K_KZG_FINISH);
  int32_t verdict = 0, fail = 1;
  M3X_HIP_CHECK(hipMemcpyAsync(&verdict, w.verdict, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
  M3X_HIP_CHECK(
      hipMemcpyAsync(&fail, w.fail, 4, hipMemcpyDeviceToHost, ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream2));
  if (fail) return M3X_ERR_ENCODING;
  *out = verdict;
  return M3X_OK;
}

bool kzg_args_ok(m3x_ctx *ctx, m3x_kzg *kzg, uint64_t n) {
  return ctx && kzg && kzg->g2 && kzg->device == ctx->device &&
         n <= KZG_MAX_BATCH;
}

// ================================================================= prover
//
// blob_to_kzg_commitment / compute_kzg_proof / compute_blob_kzg_proof: a
// 4096-term G1 multi-scalar multiplication over the fixed Lagrange basis.
// Fixed basis => no doublings and no buckets at run time: with signed
// 4-bit digits s = sum_j d_j 16^j, d_j in [-7, 8],
//   sum_i s_i L_i = sum_{i,j} sign(d_ij) * T[j][i][|d_ij| - 1]
// is 64 * 4096 table look-ups joined by mixed additions.
//   k_kzgp_bases     validate the 4096 points, bases[j][i] = [16^j] L_i
//   k_kzgp_table     d = 1..8 multiples of every base, one shared inversion
//   k_kzgp_quotient  q_i = (f_i - y)/(w_i - z), with the in-domain term
//   k_kzgp_msm       16 look-ups per lane, 16384 lanes per blob, block sum
//   k_kzgp_finish    the last 64 partial sums of a blob + g1_compress

// KZGP_WINDOWS, KZGP_DIGITS and KZGP_TABLE_POINTS: m3x_kzg.hh
#define KZGP_PER_LANE 16 // windows (look-ups) per MSM lane
#define KZGP_BLOCKS (KZG_N * (KZGP_WINDOWS / KZGP_PER_LANE) / 256)

// one lane per Lagrange point, in blob order: element e of a blob pairs
// with entry bitrev12(e) of the ceremony file's list
__global__ __launch_bounds__(64, 1) void k_kzgp_bases(
    const uint8_t *__restrict__ lagrange, g1j *__restrict__ bases,
    int *__restrict__ fail) {
  uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= KZG_N) return;
  g1a p;
  bool ok = kzg_validate_g1(p, lagrange + 48 * bitrev_lo(e, 12)) && !p.inf;
  if (!ok) {
    atomicOr(fail, 1);
    g1_gen(p); // placeholder; the load already failed
  }
  g1j b;
  g1j_from_aff(b, p);
  for (int j = 0; j < KZGP_WINDOWS; j++) {
    bases[(uint32_t)j * KZG_N + e] = b;
    for (int k = 0; k < 4; k++) g1j_dbl(b, b);
  }
}

// lane (j, i): B, 2B, ..., 8B in Jacobian form, then affine through one
// inversion of the product of the eight z (Montgomery's trick)
__global__ __launch_bounds__(64, 1) void k_kzgp_table(
    const g1j *__restrict__ bases, g1t *__restrict__ table) {
  uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= KZGP_WINDOWS * KZG_N) return;
  g1j m[KZGP_DIGITS];
  m[0] = bases[lane];
  g1j_dbl(m[1], m[0]);
  g1j_add(m[2], m[1], m[0]);
  g1j_dbl(m[3], m[1]);
  g1j_add(m[4], m[3], m[0]);
  g1j_dbl(m[5], m[2]);
  g1j_add(m[6], m[5], m[0]);
  g1j_dbl(m[7], m[3]);
  fp pre[KZGP_DIGITS];
  pre[0] = m[0].z;
  for (int d = 1; d < KZGP_DIGITS; d++) fp_mul(pre[d], pre[d - 1], m[d].z);
  fp inv;
  fp_inv(inv, pre[KZGP_DIGITS - 1]);
  for (int d = KZGP_DIGITS - 1; d >= 0; d--) {
    fp zi, zi2, zi3;
    if (d > 0)
      fp_mul(zi, inv, pre[d - 1]);
    else
      zi = inv;
    fp_mul(inv, inv, m[d].z);
    fp_sqr(zi2, zi);
    fp_mul(zi3, zi2, zi);
    g1t out;
    fp_mul(out.x, m[d].x, zi2);
    fp_mul(out.y, m[d].y, zi3);
    table[(uint64_t)lane * KZGP_DIGITS + d] = out;
  }
}

// compute_kzg_proof_impl's quotient in evaluation form, k_kzg_eval's shape
// (one block per blob, 16 elements per thread, one inversion per thread).
// z = w_m: q_m = sum_{i != m} (f_i - y) w_i / (z (z - w_i))
//              = -(1/z) sum_{i != m} q_i w_i.
// Scalars leave as canonical big-endian bytes, the blob's own format.
__global__ __launch_bounds__(256) void k_kzgp_quotient(
    const uint8_t *__restrict__ blobs, uint64_t n, KzgWork w,
    uint8_t *__restrict__ qs) {
  __shared__ fr lds[256];
  __shared__ int s_m;
  uint64_t b = blockIdx.x;
  int t = threadIdx.x;
  if (b >= n) return;
  const uint8_t *blob = blobs + b * KZG_BLOB_BYTES;
  uint8_t *q_out = qs + b * KZG_BLOB_BYTES;
  if (t == 0) s_m = -1;
  __syncthreads();
  fr z, y;
  // a non-canonical z or y was flagged by k_kzg_eval; the call has failed
  if (!fr_from_be32(z, w.zs + 32 * b)) fr_zero(z);
  if (!fr_from_be32(y, w.ys + 32 * b)) fr_zero(y);
  DomainWalk dw;
  BatchInv16 bi;
  dw.init(t);
  fr run;
  bi.init(run);
  fr num[16];
  int hit = -1;
  for (int mi = 0; mi < 16; mi++) {
    fr f, wk, d;
    uint32_t j = dw.next(mi, wk);
    if (!fr_from_be32(f, blob + 32 * j)) fr_zero(f); // flagged by k_kzg_eval
    fr_sub(d, wk, z);
    fr_sub(num[mi], f, y);
    if (fr_is_zero(d)) { // z = w_j: this element takes the in-domain term
      s_m = (int)j;
      hit = mi;
      fr_one(d);
    }
    bi.push(run, mi, d);
  }
  fr acc;
  bi.invert(run);
  fr_zero(acc);
  for (int mi = 15; mi >= 0; mi--) {
    fr id, q, wk, term;
    bi.pop(run, mi, id);
    if (mi == hit) continue;
    fr_mul(q, num[mi], id);
    fr_to_be32(q, q_out + 32 * dw.index(mi));
    fr_add(wk, bi.den[mi], z);
    fr_mul(term, q, wk);
    fr_add(acc, acc, term);
  }
  lds[t] = acc;
  block_tree_reduce<fr, 256>(lds, t, fr_add_op{});
  if (t == 0 && s_m >= 0) {
    fr zi, q;
    fr_inv(zi, z); // z is a root of unity here, never zero
    fr_mul(q, lds[0], zi);
    fr_neg(q, q);
    fr_to_be32(q, q_out + 32 * (uint32_t)s_m);
  }
}

// the MSM's look-up stage. Lane (element e, quarter q) owns windows
// 16q..16q+15 of scalar e. Signed recoding d = nibble + carry, d > 8 =>
// d - 16 and carry 1; the carry into window k is 1 exactly when the low k
// nibbles exceed 0x88..8 (the largest value k digits <= 8 can hold), so
// each quarter finds its carry-in without walking the windows below it.
// A scalar is < r < 2^255: the top nibble is <= 7 and never carries out.
// The 256 lane sums of a block are joined in LDS; every addition takes the
// doubling, inverse and infinity branches of g1j_add / g1j_add_aff.
__global__ __launch_bounds__(256) void k_kzgp_msm(
    const uint8_t *__restrict__ scalars, const g1t *__restrict__ table,
    g1j *__restrict__ partial, int *__restrict__ fail) {
  __shared__ g1j lds[256];
  uint32_t t = threadIdx.x;
  uint32_t lane = blockIdx.x * 256 + t; // < 16384
  uint32_t e = lane >> 2, q = lane & 3;
  uint64_t blob = blockIdx.y;
  uint32_t s[8];
  fr_limbs_from_be32(s, scalars + (blob * KZG_N + e) * 32);
  if (fr_ge_r(s)) { // non-canonical blob element
    if (q == 0) atomicOr(fail, 1);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = 0;
  }
  bool gt = false;
  uint32_t carry_in[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 6; i++) {
    gt = s[i] > 0x88888888u || (s[i] == 0x88888888u && gt);
    if (i & 1) carry_in[(i + 1) >> 1] = gt ? 1u : 0u;
  }
  uint32_t lo = s[0], hi = s[1], carry = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (q == (uint32_t)k) {
      lo = s[2 * k];
      hi = s[2 * k + 1];
      carry = carry_in[k];
    }
  uint64_t bits = ((uint64_t)hi << 32) | lo;
  g1j acc;
  g1j_set_inf(acc);
  for (uint32_t k = 0; k < KZGP_PER_LANE; k++) {
    int d = (int)((bits >> (4 * k)) & 15) + (int)carry;
    carry = d > 8 ? 1u : 0u;
    if (carry) d -= 16;
    if (d == 0) continue;
    uint32_t mag = (uint32_t)(d < 0 ? -d : d); // 1..8
    uint32_t j = KZGP_PER_LANE * q + k;
    const g1t &tp =
        table[((uint64_t)j * KZG_N + e) * KZGP_DIGITS + (mag - 1)];
    g1a pt;
    pt.x = tp.x;
    pt.y = tp.y;
    pt.inf = 0;
    if (d < 0) fp_neg(pt.y, pt.y);
    g1j_add_aff(acc, acc, pt);
  }
  lds[t] = acc;
  block_tree_reduce<g1j, 256>(lds, (int)t, g1j_add_op{});
  if (t == 0) partial[blob * KZGP_BLOCKS + blockIdx.x] = lds[0];
}

// one block per blob: the KZGP_BLOCKS partial sums, then the wire form
__global__ __launch_bounds__(KZGP_BLOCKS) void k_kzgp_finish(
    const g1j *__restrict__ partial, uint8_t *__restrict__ out) {
  __shared__ g1j lds[KZGP_BLOCKS];
  uint32_t t = threadIdx.x;
  uint64_t blob = blockIdx.x;
  lds[t] = partial[blob * KZGP_BLOCKS + t];
  block_tree_reduce<g1j, KZGP_BLOCKS>(lds, (int)t, g1j_add_op{});
  if (t == 0) g1_compress(out + 48 * blob, lds[0]);
}

// commitment validation for compute_blob_kzg_proof: one lane per point
__global__ __launch_bounds__(64, 1) void k_kzgp_check_g1(
    const uint8_t *__restrict__ cs, uint64_t n, int *__restrict__ fail) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  g1a p;
  if (!kzg_validate_g1(p, cs + 48 * lane)) atomicOr(fail, 1);
}

struct KzgpWork {
  uint8_t *qs;   // [n*131072] quotient scalars, canonical BE
  g1j *partial;  // [n*KZGP_BLOCKS] block sums of the MSM
};

int kzgp_layout(m3x_ctx *ctx, uint64_t n, bool quotient, KzgpWork &p) {
  return m3x::carve_scratch(
      ctx, &ctx->scratch_b, &ctx->scratch_b_bytes, [&](m3x::ScratchCarver &c) {
        p.partial = c.take<g1j>(n * KZGP_BLOCKS);
        p.qs = c.take<uint8_t>(quotient ? n * KZG_BLOB_BYTES : 0);
      });
}

bool kzgp_args_ok(m3x_ctx *ctx, m3x_kzg *kzg, uint64_t n) {
  return kzg_args_ok(ctx, kzg, n) && kzg->table;
}

// n MSMs over the handle's table: scalars_dev n*4096*32 BE, out_dev n*48
void launch_msm(m3x_ctx *ctx, m3x_kzg *kzg, const KzgWork &w,
                const KzgpWork &p, const uint8_t *scalars_dev, uint64_t n,
                uint8_t *out_dev) {
  m3x::time_begin(ctx, M3X_K_KZGP_MSM);
  hipLaunchKernelGGL(k_kzgp_msm, dim3(KZGP_BLOCKS, (uint32_t)n), dim3(256), 0,
                     ctx->stream, scalars_dev, kzg->table, p.partial, w.fail);
  m3x::time_end(ctx, M3X_K_KZGP_MSM);
  m3x::time_begin(ctx, M3X_K_KZGP_FINISH);
  hipLaunchKernelGGL(k_kzgp_finish, dim3((uint32_t)n), dim3(KZGP_BLOCKS), 0,
                     ctx->stream, p.partial, out_dev);
  m3x::time_end(ctx, M3X_K_KZGP_FINISH);
}

// quotient + MSM once w.zs and w.ys hold z and y
void launch_quotient_msm(m3x_ctx *ctx, m3x_kzg *kzg, const KzgWork &w,
                         const KzgpWork &p, const uint8_t *blobs_dev,
                         uint64_t n, uint8_t *out_dev) {
  m3x::time_begin(ctx, M3X_K_KZGP_QUOTIENT);
  hipLaunchKernelGGL(k_kzgp_quotient, dim3((uint32_t)n), dim3(256), 0,
                     ctx->stream, blobs_dev, n, w, p.qs);
  m3x::time_end(ctx, M3X_K_KZGP_QUOTIENT);
  launch_msm(ctx, kzg, w, p, p.qs, n, out_dev);
}

// read the failure flag back after everything queued on the main stream
int kzgp_wait(m3x_ctx *ctx, const KzgWork &w) {
  int32_t fail = 1;
  M3X_HIP_CHECK(
      hipMemcpyAsync(&fail, w.fail, 4, hipMemcpyDeviceToHost, ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

} // namespace

// the kernels the cell pipeline reuses (declared in m3x_kzg.hh)
namespace m3x {
void launch_kzg_setup(hipStream_t st, const uint8_t *g2_96_dev, g2j *out,
                      int *fail) {
  hipLaunchKernelGGL(k_kzg_setup, dim3(1), dim3(1), 0, st, g2_96_dev, out,
                     fail);
}

void launch_kzg_sum_g1(hipStream_t st, const g1j *in, uint64_t n, g1j *stage,
                       g1j *out, const int *fail) {
  uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(blocks), dim3(256), 0, st, in, n,
                     stage, fail);
  hipLaunchKernelGGL(k_kzg_reduce_g1, dim3(1), dim3(256), 0, st, stage,
                     (uint64_t)blocks, out, fail);
}

void launch_kzg_finish(hipStream_t st, g1j *sums, int *fail, int *verdict,
                       const g2j *g2) {
  KzgWork w{};
  w.sums = sums;
  w.fail = fail;
  w.verdict = verdict;
  hipLaunchKernelGGL(k_kzg_finish, dim3(1), dim3(64), 0, st, w, g2);
}

void launch_kzgp_bases(hipStream_t st, const uint8_t *points_dev, g1j *bases,
                       int *fail) {
  hipLaunchKernelGGL(k_kzgp_bases, dim3(KZG_N / 64), dim3(64), 0, st,
                     points_dev, bases, fail);
}

void launch_kzgp_table(hipStream_t st, const g1j *bases, g1t *table) {
  hipLaunchKernelGGL(k_kzgp_table, dim3(KZGP_WINDOWS * KZG_N / 64), dim3(64),
                     0, st, bases, table);
}
} // namespace m3x

extern "C" {

int32_t m3x_kzg_create(m3x_ctx *ctx, const uint8_t g2_tau[96],
                       m3x_kzg **out) {
  if (!ctx || !g2_tau || !out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  g2j *g2 = tmp.alloc<g2j>(2 * sizeof(g2j));
  const uint8_t *tau_d = tmp.upload(g2_tau, 96);
  int *fail_d = tmp.alloc<int>(4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  hipLaunchKernelGGL(k_kzg_setup, dim3(1), dim3(1), 0, ctx->stream, tau_d, g2,
                     fail_d);
  int fail = 1;
  tmp.download(&fail, fail_d, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail) return M3X_ERR_ENCODING;
  auto *k = new m3x_kzg();
  k->device = ctx->device;
  k->g2 = tmp.release(g2); // the handle owns it from here
  *out = k;
  return M3X_OK;
}

void m3x_kzg_destroy(m3x_kzg *kzg) {
  if (!kzg) return;
  if (hipSetDevice(kzg->device) == hipSuccess) {
    if (kzg->g2) (void)hipFree(kzg->g2);
    if (kzg->table) (void)hipFree(kzg->table);
    if (kzg->cell_g1) (void)hipFree(kzg->cell_g1);
    if (kzg->cell_g2) (void)hipFree(kzg->cell_g2);
    if (kzg->mono_table) (void)hipFree(kzg->mono_table);
  }
  delete kzg;
}

int32_t m3x_kzgp_load_g1_lagrange(m3x_ctx *ctx, m3x_kzg *kzg,
                                  const uint8_t *g1_lagrange) {
  if (!kzg_args_ok(ctx, kzg, 0) || !g1_lagrange || kzg->table)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *lag_d = tmp.upload(g1_lagrange, (uint64_t)KZG_N * 48);
  int *fail_d = tmp.alloc<int>(4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  g1j *bases = tmp.alloc<g1j>((uint64_t)KZGP_WINDOWS * KZG_N * sizeof(g1j));
  g1t *table = tmp.alloc<g1t>(KZGP_TABLE_POINTS * sizeof(g1t));
  if (!tmp.ok()) return M3X_ERR_NOMEM;
  M3X_HIP_CHECK(hipMemsetAsync(fail_d, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_kzgp_bases, dim3(KZG_N / 64), dim3(64), 0, ctx->stream,
                     lag_d, bases, fail_d);
  int fail = 1;
  tmp.download(&fail, fail_d, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail) return M3X_ERR_ENCODING;
  hipLaunchKernelGGL(k_kzgp_table, dim3(KZGP_WINDOWS * KZG_N / 64), dim3(64),
                     0, ctx->stream, bases, table);
  if (!tmp.sync()) return M3X_ERR_HIP;
  kzg->table = tmp.release(table); // the handle owns it from here
  return M3X_OK;
}

int32_t m3x_kzgp_blob_to_commitment_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const void *blobs_dev, uint64_t n,
                                        void *out_dev) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs_dev || !out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  KzgWork w;
  KzgpWork p;
  int rc = kzg_layout(ctx, n, w);
  if (rc == M3X_OK) rc = kzgp_layout(ctx, n, false, p);
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  // the MSM digits come straight from the blob bytes
  launch_msm(ctx, kzg, w, p, (const uint8_t *)blobs_dev, n,
             (uint8_t *)out_dev);
  return kzgp_wait(ctx, w);
}

int32_t m3x_kzgp_blob_to_commitment(m3x_ctx *ctx, m3x_kzg *kzg,
                                    const uint8_t *blobs, uint64_t n,
                                    uint8_t *out) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs || !out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES);
  uint8_t *out_d = tmp.alloc(n * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t rc = m3x_kzgp_blob_to_commitment_dev(ctx, kzg, bl_d, n, out_d);
  if (rc != M3X_OK) return rc;
  tmp.download(out, out_d, n * 48);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_kzgp_compute_proof_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                   const void *blobs_dev, const void *zs_dev,
                                   uint64_t n, void *proofs_out_dev,
                                   void *ys_out_dev) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs_dev || !zs_dev || !proofs_out_dev || !ys_out_dev)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  KzgWork w;
  KzgpWork p;
  int rc = kzg_layout(ctx, n, w);
  if (rc == M3X_OK) rc = kzgp_layout(ctx, n, true, p);
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  rc = launch_challenge_eval(ctx, w, (const uint8_t *)blobs_dev, nullptr,
                             (const uint8_t *)zs_dev, n);
  if (rc != M3X_OK) return rc;
  launch_quotient_msm(ctx, kzg, w, p, (const uint8_t *)blobs_dev, n,
                      (uint8_t *)proofs_out_dev);
  M3X_HIP_CHECK(hipMemcpyAsync(ys_out_dev, w.ys, n * 32,
                               hipMemcpyDeviceToDevice, ctx->stream));
  return kzgp_wait(ctx, w);
}

int32_t m3x_kzgp_compute_proof(m3x_ctx *ctx, m3x_kzg *kzg,
                               const uint8_t *blobs, const uint8_t *zs,
                               uint64_t n, uint8_t *proofs_out,
                               uint8_t *ys_out) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs || !zs || !proofs_out || !ys_out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES);
  const uint8_t *zs_d = tmp.upload(zs, n * 32);
  uint8_t *pr_d = tmp.alloc(n * 48), *ys_d = tmp.alloc(n * 32);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t rc = m3x_kzgp_compute_proof_dev(ctx, kzg, bl_d, zs_d, n, pr_d, ys_d);
  if (rc != M3X_OK) return rc;
  tmp.download(proofs_out, pr_d, n * 48);
  tmp.download(ys_out, ys_d, n * 32);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_kzgp_compute_blob_proof_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const void *blobs_dev,
                                        const void *cs_dev, uint64_t n,
                                        void *out_dev) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs_dev || !cs_dev || !out_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  KzgWork w;
  KzgpWork p;
  int rc = kzg_layout(ctx, n, w);
  if (rc == M3X_OK) rc = kzgp_layout(ctx, n, true, p);
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  // the commitment check feeds nothing but the failure flag: it runs on
  // stream3 beside the whole challenge -> eval -> quotient -> MSM chain
  M3X_HIP_CHECK(hipEventRecord(ctx->ev_pipe[0], ctx->stream));
  M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream3, ctx->ev_pipe[0], 0));
  m3x::time_begin_s(ctx, M3X_K_KZG_DECOMP, ctx->stream3);
  hipLaunchKernelGGL(k_kzgp_check_g1, dim3((uint32_t)((n + 63) / 64)),
                     dim3(64), 0, ctx->stream3, (const uint8_t *)cs_dev, n,
                     w.fail);
  m3x::time_end_s(ctx, M3X_K_KZG_DECOMP, ctx->stream3);
  M3X_HIP_CHECK(hipEventRecord(ctx->ev_pipe[1], ctx->stream3));
  rc = launch_challenge_eval(ctx, w, (const uint8_t *)blobs_dev,
                             (const uint8_t *)cs_dev, nullptr, n);
  if (rc == M3X_OK)
    launch_quotient_msm(ctx, kzg, w, p, (const uint8_t *)blobs_dev, n,
                        (uint8_t *)out_dev);
  if (hipStreamWaitEvent(ctx->stream, ctx->ev_pipe[1], 0) != hipSuccess)
    rc = M3X_ERR_HIP;
  int rc2 = kzgp_wait(ctx, w);
  (void)hipStreamSynchronize(ctx->stream2);
  (void)hipStreamSynchronize(ctx->stream3);
  return rc != M3X_OK ? rc : rc2;
}

int32_t m3x_kzgp_compute_blob_proof(m3x_ctx *ctx, m3x_kzg *kzg,
                                    const uint8_t *blobs, const uint8_t *cs,
                                    uint64_t n, uint8_t *out) {
  if (!kzgp_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  if (!blobs || !cs || !out) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES);
  const uint8_t *cs_d = tmp.upload(cs, n * 48);
  uint8_t *out_d = tmp.alloc(n * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  // synchronises stream2 and stream3 itself, also when it fails
  int32_t rc = m3x_kzgp_compute_blob_proof_dev(ctx, kzg, bl_d, cs_d, n, out_d);
  if (rc != M3X_OK) return rc;
  tmp.download(out, out_d, n * 48);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_kzg_verify_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                   const uint8_t *cs, const uint8_t *zs,
                                   const uint8_t *ys, const uint8_t *proofs,
                                   uint64_t n) {
  if (!kzg_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return 1;
  if (!cs || !zs || !ys || !proofs) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *cs_d = tmp.upload(cs, n * 48), *zs_d = tmp.upload(zs, n * 32),
                *ys_d = tmp.upload(ys, n * 32),
                *pr_d = tmp.upload(proofs, n * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int32_t verdict = 0;
  int32_t rc = run_kzg(ctx, kzg, nullptr, cs_d, zs_d, ys_d, pr_d, n, &verdict);
  return rc == M3X_OK ? verdict : rc;
}

int32_t m3x_kzg_verify_proof(m3x_ctx *ctx, m3x_kzg *kzg, const uint8_t c[48],
                             const uint8_t z[32], const uint8_t y[32],
                             const uint8_t proof[48]) {
  return m3x_kzg_verify_proof_batch(ctx, kzg, c, z, y, proof, 1);
}

int32_t m3x_kzg_verify_blob_proof_batch_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                            const void *blobs_dev,
                                            const void *cs_dev,
                                            const void *proofs_dev,
                                            uint64_t n) {
  if (!kzg_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return 1;
  if (!blobs_dev || !cs_dev || !proofs_dev) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  int32_t verdict = 0;
  int rc = run_kzg(ctx, kzg, (const uint8_t *)blobs_dev,
                   (const uint8_t *)cs_dev, nullptr, nullptr,
                   (const uint8_t *)proofs_dev, n, &verdict);
  return rc == M3X_OK ? verdict : rc;
}

int32_t m3x_kzg_verify_blob_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const uint8_t *blobs,
                                        const uint8_t *cs,
                                        const uint8_t *proofs, uint64_t n) {
  if (!kzg_args_ok(ctx, kzg, n)) return M3X_ERR_ARG;
  if (n == 0) return 1;
  if (!blobs || !cs || !proofs) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES),
                *cs_d = tmp.upload(cs, n * 48),
                *pr_d = tmp.upload(proofs, n * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  return m3x_kzg_verify_blob_proof_batch_dev(ctx, kzg, bl_d, cs_d, pr_d, n);
}

int32_t m3x_kzg_blob_challenge_eval(m3x_ctx *ctx, const uint8_t *blobs,
                                    const uint8_t *cs, const uint8_t *zs_in,
                                    uint64_t n, uint8_t *out_z,
                                    uint8_t *out_y) {
  if (!ctx || !blobs || !cs || !out_z || !out_y || n == 0 ||
      n > KZG_MAX_BATCH)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  KzgWork w;
  int32_t rc = kzg_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *bl_d = tmp.upload(blobs, n * KZG_BLOB_BYTES),
                *cs_d = tmp.upload(cs, n * 48),
                *zs_d = zs_in ? tmp.upload(zs_in, n * 32) : nullptr;
  if (!tmp.ok()) return M3X_ERR_HIP;
  int fail = 1;
  bool queued = hipMemsetAsync(w.fail, 0, 4, ctx->stream) == hipSuccess &&
                launch_challenge_eval(ctx, w, bl_d, cs_d, zs_d, n) == M3X_OK;
  if (queued) {
    tmp.download(out_z, w.zs, n * 32);
    tmp.download(out_y, w.ys, n * 32);
    tmp.download(&fail, w.fail, 4);
  }
  // on failure too: nothing is freed while stream2 may still read the blobs
  (void)hipStreamSynchronize(ctx->stream2);
  if (!tmp.sync() || !queued) return M3X_ERR_HIP;
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

int32_t m3x_kzg_batch_challenge_test(m3x_ctx *ctx, const uint8_t *cs,
                                     const uint8_t *zs, const uint8_t *ys,
                                     const uint8_t *proofs, uint64_t n,
                                     uint8_t out_r[32]) {
  if (!ctx || !cs || !zs || !ys || !proofs || !out_r || n == 0 ||
      n > KZG_MAX_BATCH)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  KzgWork w;
  int32_t rc = kzg_layout(ctx, n, w);
  if (rc != M3X_OK) return rc;
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *cs_d = tmp.upload(cs, n * 48),
                *pr_d = tmp.upload(proofs, n * 48);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int fail = 1;
  bool queued =
      hipMemsetAsync(w.fail, 0, 4, ctx->stream) == hipSuccess &&
      hipMemcpyAsync(w.zs, zs, n * 32, hipMemcpyHostToDevice, ctx->stream) ==
          hipSuccess &&
      hipMemcpyAsync(w.ys, ys, n * 32, hipMemcpyHostToDevice, ctx->stream) ==
          hipSuccess;
  if (queued) {
    hipLaunchKernelGGL(k_kzg_batch_r, dim3(1), dim3(256), 0, ctx->stream, cs_d,
                       pr_d, n, w);
    tmp.download(out_r, w.r_out, 32);
    tmp.download(&fail, w.fail, 4);
  }
  if (!tmp.sync() || !queued) return M3X_ERR_HIP;
  return fail ? M3X_ERR_ENCODING : M3X_OK;
}

} // extern "C"
