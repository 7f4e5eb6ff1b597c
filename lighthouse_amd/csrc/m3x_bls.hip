// MI355X-native batched BLS12-381 signature-set verification (hot path #1).
//
// Implements the blst.rs:37-119 contract (see include/m3x_consensus.h and
// DESIGN.md): per set — decompress + subgroup-check sigma (deferred checks
// exactly as generic_aggregate_signature.rs:161-176 + blst.rs:73-77),
// aggregate the set's pubkeys, scale by the host-drawn 64-bit r_i, hash the
// message to G2 (RFC 9380), accumulate one Miller loop per set; then one
// extra pair e(-g1, sum r_i sigma_i), one final exponentiation, compare to
// one. CDNA4 shape: one set per lane, kernels split by divergence class,
// grids ≫256 workgroups; integer VALU workload (no MFMA).
#include "bls_device.hh"
#include "m3x_ctx.hh"
#include "../../include/m3x_consensus.h"
#include <cstdio>
#include <cstdlib>

// M3X_DEBUG_SYNC=1: synchronize + trace after each BLS kernel (debug aid)
static bool dbg_sync() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("M3X_DEBUG_SYNC");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
#define DBG_STEP(ctx, name)                                                    \
  do {                                                                         \
    if (dbg_sync()) {                                                          \
      hipError_t _e = hipStreamSynchronize((ctx)->stream);                     \
      fprintf(stderr, "[m3x dbg] %s: %s\n", name, hipGetErrorString(_e));      \
      fflush(stderr);                                                          \
    }                                                                          \
  } while (0)

using namespace m3xb;

namespace {

struct BlsWork {
  g1j *apk;        // [n] precomputed aggregate pubkeys (k>1 sets)
  uint64_t *agg_idx; // [n] indices of k>1 sets (count in agg_count[0])
  uint32_t *agg_count;
  g1j *p_scaled;   // [n] r_i * aggregate pubkey (Jacobian)
  g2j *h2c;        // [n] hash_to_curve(msg), Jacobian (no inversion)
  uint8_t *uni;    // [n*256] expand_message_xmd output (h2c pass 1)
  g2j *h2c_pts;    // [2n] per-point sswu+iso outputs (h2c pass 2)
  g2j *rsig;       // [n] r_i * sigma (jacobian)
  g2j *sig_aff;    // [n] decompressed sigma (z=1 affine; z=0 infinity)
  fp12m *fparts;   // [n] per-set miller values
  int *fail;       // [1]
  g2j *sig_stage;  // [256] stage-1 partial sums
  g2j *sig_sum;    // [1]
  fp12m *gt_stage; // [256] stage-1 partial products
  fp12m *gt_parts; // [1]
  fp12m *sig_gt;   // [1] miller(-g1, sig_sum), written by the side stream
  int *verdict;    // [1]
  m3x::SigMsmWork msm; // bucket-MSM form of the signature sum
};

// Where a stage records a malformed input. The batch pipeline has one flag
// per call: any bad set makes the batch false. The per-set pipeline
// (m3x_bls_verify_each) marks only the set the input belongs to, so a bad
// set never changes another set's verdict.
struct BatchFail {
  int *flag;
  __device__ __forceinline__ void mark(uint64_t) const { atomicOr(flag, 1); }
};
struct SetFail {
  int32_t *status; // [n], zeroed per call; non-zero = verdict forced to 0
  __device__ __forceinline__ void mark(uint64_t set) const {
    atomicOr(&status[set], 1);
  }
};

// ---------------------------------------------------------------- kernels

__global__ __launch_bounds__(64, 1) void k_bls_pk_decompress(const uint8_t *__restrict__ comp,
                                    uint64_t n, uint8_t *__restrict__ uncomp,
                                    int32_t *__restrict__ status) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1a p;
  if (g1_decompress(p, comp + 48 * i) != 0) {
    status[i] = -1;
    return;
  }
  if (p.inf) { // infinity pubkey rejected (generic_public_key.rs:86-94)
    status[i] = -2;
    return;
  }
  if (!g1_in_subgroup(p)) {
    status[i] = -4;
    return;
  }
  g1_to_uncomp(p, uncomp + 96 * i);
  status[i] = 0;
}

// collect the k>1 sets (their aggregation runs wave-parallel)
__global__ void k_bls_scan_agg(const uint32_t *__restrict__ offs, uint64_t n,
                               BlsWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (offs[i + 1] - offs[i] > 1) {
    uint32_t pos = atomicAdd(w.agg_count, 1u);
    w.agg_idx[pos] = i;
  }
}

// grid cap of k_bls_aggregate_w (its blocks stride over the k>1 sets)
constexpr uint32_t kAggMaxBlocks = 32768;

// one WAVE per k>1 set: each lane partial-sums a strided slice of the
// set's pubkeys in Jacobian form, then an LDS tree reduce (6 levels)
template <typename Fail>
__device__ __forceinline__ void aggregate_w_body(
    const uint8_t *__restrict__ pks, const uint32_t *__restrict__ offs,
    const BlsWork &w, g1j *lds, Fail fail) {
  // grid-stride over the aggregate list: the grid is CAPPED (at
  // kAggMaxBlocks) so a k=1-only workload costs ~nothing — launching n
  // blocks of early-exits measured 183 ms at n=1M (rocprof r02)
  for (uint32_t b = blockIdx.x; b < *w.agg_count; b += gridDim.x) {
  uint64_t set = w.agg_idx[b];
  uint32_t k0 = offs[set], k1 = offs[set + 1];
  int lane = threadIdx.x;
  g1j acc;
  g1j_set_inf(acc);
  bool bad = false;
  for (uint32_t k = k0 + lane; k < k1; k += 64) {
    g1a pk;
    if (g1_from_uncomp_trusted(pk, pks + 96 * (uint64_t)k) != 0) {
      bad = true;
      break;
    }
    g1j_add_aff(acc, acc, pk);
  }
  if (bad) fail.mark(set);
  lds[lane] = acc;
  block_tree_reduce<g1j, 64>(lds, lane, g1j_add_op{});
  if (lane == 0) w.apk[set] = lds[0];
  __syncthreads(); // next grid-stride iteration reuses lds
  }
}

__global__ __launch_bounds__(64, 1) void k_bls_aggregate_w(
    const uint8_t *__restrict__ pks, const uint32_t *__restrict__ offs,
    BlsWork w) {
  __shared__ g1j lds[64];
  aggregate_w_body(pks, offs, w, lds, BatchFail{w.fail});
}

// per-set twin: a pubkey that does not parse marks its own set (the sum of
// the keys that did parse is still stored, a well-formed point)
__global__ __launch_bounds__(64, 1) void k_bls_aggregate_w_each(
    const uint8_t *__restrict__ pks, const uint32_t *__restrict__ offs,
    BlsWork w, int32_t *__restrict__ status) {
  __shared__ g1j lds[64];
  aggregate_w_body(pks, offs, w, lds, SetFail{status});
}

// FUSED per-set prepare (kept for LARGE batches): at high occupancy the
// kernel is ISSUE-bound and the shared-doubling dual-scalar chain does
// less total work than the split form (rocprof r02g: 450 vs 657+116 ms
// at 1M sets); the split form wins in the small-batch LATENCY regime
// (32 vs 37 ms at 64k). Dispatch picks by n.
__global__ __launch_bounds__(64, 1) void k_bls_prepare(const uint8_t *__restrict__ sigs,
                              const uint8_t *__restrict__ pks,
                              const uint32_t *__restrict__ offs,
                              const uint64_t *__restrict__ rands, uint64_t n,
                              BlsWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2a sig;
  if (g2_decompress(sig, sigs + 96 * i) != 0) {
    atomicOr(w.fail, 1);
    return;
  }
  uint32_t k0 = offs[i], k1 = offs[i + 1];
  if (k1 <= k0) {
    atomicOr(w.fail, 1);
    return;
  }
  g1j apk;
  if (k1 - k0 == 1) {
    g1a pk;
    if (g1_from_uncomp_trusted(pk, pks + 96 * (uint64_t)k0) != 0) {
      atomicOr(w.fail, 1);
      return;
    }
    g1j_from_aff(apk, pk);
  } else {
    apk = w.apk[i]; // precomputed by k_bls_aggregate_w
  }
  if (g1j_is_inf(apk)) { // aggregate at infinity -> invalid
    atomicOr(w.fail, 1);
    return;
  }
  uint8_t rbe[8];
#pragma unroll
  for (int b = 0; b < 8; b++) rbe[b] = (uint8_t)(rands[i] >> (56 - 8 * b));
  g1j rp;
  g1j_mul_be_j(rp, apk, rbe, 8); // P stays Jacobian end-to-end
  w.p_scaled[i] = rp;
  if (sig.inf) {
    // infinity is a valid subgroup element; contributes nothing
    g2j_set_inf(w.rsig[i]);
  } else {
    // [r]sigma and the psi subgroup check's [|x|]sigma share sigma's
    // doubling chain (blst.rs:73-77 deferred subgroup check)
    g2j rsig_j, xsig_j;
    g2j_mul2_u64(rsig_j, xsig_j, sig, rands[i], BLS_X_ABS);
    w.rsig[i] = rsig_j;
    if (!psi_eq_neg(sig, xsig_j)) atomicOr(w.fail, 1);
  }
}

// [k]B for an affine G2 base with MIXED adds (24 vs 43 fp-muls per add);
// MSB-first double-and-add. Separate per-scalar chains with mixed adds
// cost LESS total than the round-1 shared-doubling chain of FULL adds.
__device__ inline void g2_mul_u64_aff(g2j &r, const g2a &base, uint64_t k) {
  g2j acc;
  g2j_set_inf(acc);
  for (int b = 63; b >= 0; b--) {
    g2j_dbl(acc, acc);
    if ((k >> b) & 1) g2j_add_aff(acc, acc, base);
  }
  r = acc;
}

// [k]B for an affine G1 base with mixed adds
__device__ inline void g1_mul_u64_aff(g1j &r, const g1a &base, uint64_t k) {
  g1j acc;
  g1j_set_inf(acc);
  for (int b = 63; b >= 0; b--) {
    g1j_dbl(acc, acc);
    if ((k >> b) & 1) g1j_add_aff(acc, acc, base);
  }
  r = acc;
}

__global__ __launch_bounds__(64, 1) void k_bls_h2c(const uint8_t *__restrict__ msgs, uint64_t n,
                          BlsWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  m3xb::h2c_g2(w.h2c[i], msgs + 32 * i);
}

// ---- WAVE-SPLIT h2c (round 2): three passes so the heavy SSWU work runs
// at 2n lanes (2 waves/SIMD at the C2 shape) and each lane's dependent
// chain is one point, not two ----
__global__ __launch_bounds__(64, 1) void k_bls_h2c_expand(
    const uint8_t *__restrict__ msgs, uint64_t n, BlsWork w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  expand_message_xmd32(msgs + 32 * i, w.uni + 256 * i);
}

__device__ __forceinline__ void h2c_map_lane(uint64_t n, const BlsWork &w) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * n) return;
  int role = lane < n ? 0 : 1; // which of the two RO points
  uint64_t i = role == 0 ? lane : lane - n;
  const uint8_t *uni = w.uni + 256 * i + 128 * role;
  fp2 u;
  h2f_from_be64(u.c0, uni);
  h2f_from_be64(u.c1, uni + 64);
  g2a q;
  sswu_g2(q, u);
  g2j pt;
  iso_map_g2_j(pt, q);
  // not cleared here: cofactor clearing is a homomorphism, so the fin pass
  // clears the sum of the two points once. (Clearing each point at 2n
  // lanes halved the per-lane chain but doubled the ~2,700-multiply clear;
  // with the front of the step throughput-bound that lost: DESIGN.md.)
  w.h2c_pts[lane] = pt;
}

// default register budget: the high-occupancy regime (n > latency_max)
__global__ __launch_bounds__(64, 2) void k_bls_h2c_map(uint64_t n,
                                                       BlsWork w) {
  h2c_map_lane(n, w);
}

// LATENCY-REGIME register-budget twin (as k_bls_sigdec_lat and
// k_bls_prep_mults3 are): at n <= latency_max these kernels run 1-2
// waves/SIMD, so granting each wave the idle register file (512 or 256
// VGPRs vs the ~130 the default allocation picks) trades nothing and
// removes scratch spill round-trips from the serial chains.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_h2c_map_lat(uint64_t n, BlsWork w) {
  h2c_map_lane(n, w);
}

// fin pass, n lanes: the sum of a message's two iso-mapped points, then
// the one cofactor clear (two [|x|] chains with a Jacobian base)
__device__ __forceinline__ void h2c_fin_lane(uint64_t n, const BlsWork &w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2j s = w.h2c_pts[i];
  g2j_add(s, s, w.h2c_pts[n + i]);
  g2j cleared;
  clear_cofactor_g2j(cleared, s);
  w.h2c[i] = cleared;
}

__global__ __launch_bounds__(64, 1) void k_bls_h2c_fin(uint64_t n,
                                                       BlsWork w) {
  h2c_fin_lane(n, w);
}

// latency-regime register-budget twin (see k_bls_h2c_map_lat)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_h2c_fin_lat(uint64_t n, BlsWork w) {
  h2c_fin_lane(n, w);
}

// small-batch variant: ONE WAVE PER SET (cooperative miller_w). At tiny n
// (block import: ~131 sets) the per-lane kernel is latency-bound — a
// single set's serial Miller loop is tens of ms on one lane — while n
// cooperative waves spread across 256 CUs cut that ~10x. Crossover is
// empirical (M3X_SMALL_MILLER sets the threshold).
__global__ __launch_bounds__(64) void k_bls_miller_small(uint64_t n,
                                                         BlsWork w) {
  __shared__ fp12m f;
  __shared__ f12w_ws ws;
  __shared__ miller_ws mws;
  uint64_t i = blockIdx.x;
  int lane = threadIdx.x;
  if (i >= n) return;
  if (*w.fail) {
    if (lane == 0) f12_one(w.fparts[i]);
    return;
  }
  miller_w(f, w.p_scaled[i], w.h2c[i], ws, mws, lane);
  __syncthreads();
  if (lane == 0) w.fparts[i] = f;
}

__global__ __launch_bounds__(64, 1) void k_bls_miller(uint64_t n, BlsWork w) {
  // fp12 state stays in thread-local scratch: an LDS-resident variant
  // measured 2x SLOWER (123ms vs 63ms on C2) — the L1/L2-cached spill
  // traffic beats per-limb ds_read latency for this access pattern.
  // (An in-wave LDS tree fold of the 64 per-set values also regressed:
  // +5ms in the kernel and the 64x-smaller reduce became LATENCY-bound
  // at 4 blocks — reverted; measured round 2.)
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12m f;
  if (*w.fail == 0)
    miller_raw(f, w.p_scaled[i], w.h2c[i]);
  else
    f12_one(f);
  w.fparts[i] = f;
}

// WAVE-SPLIT variant (round 2): 2n lanes — lane i = set i's high bit-half,
// lane n+i = set i's low half. Doubles the wave count (2/SIMD at the C2
// 64k-set shape) and halves each lane's dependent chain; the 2n partial
// products feed the same GT reduction (their product = the n full
// Millers' product). Each wave is role-uniform: no intra-wave divergence.
__global__ __launch_bounds__(64, 2)
__attribute__((amdgpu_waves_per_eu(2))) void k_bls_miller_split(
    uint64_t n, BlsWork w) {
  // launch_bounds min-waves 2: cap the allocation at 256 VGPRs so the two
  // half-Miller waves of a SIMD actually co-reside (the whole point of
  // the split; at the default the allocator takes 511 -> 1 wave/SIMD)
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * n) return;
  int role = lane < n ? 0 : 1;
  uint64_t i = role == 0 ? lane : lane - n;
  fp12m f;
  if (*w.fail == 0)
    miller_half(f, w.p_scaled[i], w.h2c[i], role);
  else
    f12_one(f);
  w.fparts[lane] = f;
}

// Threads per block of the two batch reductions. 128 keeps the LDS of one
// GT block (128 x 576 B) plus one signature block (128 x 288 B) at 108 KiB,
// under the CU's 160 KiB, so blocks of the two chains — which run on two
// streams — can share a CU; a block is two waves, so the pair also fits on
// separate SIMDs whatever their register budgets.
constexpr int kReduceThreads = 128;
// Stage-1 block cap (= the capacity of the gt_stage / sig_stage buffers).
constexpr uint32_t kReduceMaxBlocks = 256;

// two-stage GT-product reduction: each block folds its contiguous span of
// per-set miller values (thread-strided local products, then an LDS tree)
// into one output element; a second 1-block launch folds the partials.
// A thread starts from its first element (no multiply by one); only a
// thread with no element contributes one.
__global__ __launch_bounds__(kReduceThreads) void k_bls_reduce_gt(
    const fp12m *__restrict__ in, uint64_t n, fp12m *__restrict__ out) {
  __shared__ fp12m lds[kReduceThreads];
  block_span_reduce<fp12m, kReduceThreads>(
      in, n, out, lds,
      [](fp12m &r, const fp12m &a, const fp12m &b) { f12_mul_nn(r, a, b); },
      [](fp12m &r) { f12_one(r); });
}

// two-stage sum of r_i*sigma_i, same shape (a thread with no element
// contributes infinity)
__global__ __launch_bounds__(kReduceThreads) void k_bls_reduce_sig(
    const g2j *__restrict__ in, uint64_t n, g2j *__restrict__ out) {
  __shared__ g2j lds[kReduceThreads];
  block_span_reduce<g2j, kReduceThreads>(in, n, out, lds, g2j_add_op{},
                                         [](g2j &r) { g2j_set_inf(r); });
}

// signature pair: sig_gt = miller(-g1, sig_sum), one cooperative wave.
// Runs on the side stream next to the GT reduction (it needs nothing from
// the per-set Miller kernel). A failed batch or an infinite signature sum
// gives one: e(., O) = 1.
__global__ __launch_bounds__(64) void k_bls_sigpair(BlsWork w) {
  __shared__ fp12m f;
  __shared__ f12w_ws ws;
  __shared__ miller_ws mws;
  int lane = threadIdx.x;
  if (*w.fail) {
    if (lane == 0) f12_one(w.sig_gt[0]);
    return;
  }
  g1j ng1;
  {
    g1a g;
    g1_gen(g);
    ng1.x = g.x;
    fp_neg(ng1.y, g.y);
    fp_one(ng1.z);
  }
  // sig_sum stays Jacobian: the Q-Jacobian Miller loop needs no inversion
  // (and returns one for an infinite Q)
  miller_w(f, ng1, w.sig_sum[0], ws, mws, lane);
  f12w_sync();
  f12_copy_w(w.sig_gt[0], f, lane);
}

// final: f_total = gt_parts * sig_gt; final_exp; compare to one.
// One wave, cooperative fp12 ops in LDS (the per-batch serial tail: the
// 36 coefficient products of each Fp12 multiply fan across lanes).
__global__ __launch_bounds__(64) void k_bls_finish(BlsWork w) {
  __shared__ fp12m sh[7];
  __shared__ f12w_ws ws;
  int lane = threadIdx.x;
  if (*w.fail) {
    if (lane == 0) *w.verdict = 0;
    return;
  }
  f12_copy_w(sh[0], w.gt_parts[0], lane);
  f12_copy_w(sh[1], w.sig_gt[0], lane);
  f12_mul_w(sh[1], sh[0], sh[1], ws, lane); // f_total
  final_exp_w(sh[2], sh[1], &sh[3], ws, lane);
  if (lane == 0) *w.verdict = f12_is_one(sh[2]) ? 1 : 0;
}

// one wave aggregates n compressed signatures: lane-strided decompress +
// Jacobian partial sums, LDS tree reduce, lane 0 compresses the total
__global__ __launch_bounds__(64, 1) void k_bls_sig_aggregate_w(
    const uint8_t *__restrict__ sigs, uint64_t n, uint8_t *__restrict__ out,
    int *__restrict__ fail) {
  __shared__ g2j lds[64];
  int lane = threadIdx.x;
  g2j acc;
  g2j_set_inf(acc);
  bool bad = false;
  for (uint64_t i = lane; i < n; i += 64) {
    g2a sg;
    if (g2_decompress(sg, sigs + 96 * i) != 0) {
      bad = true;
      break;
    }
    if (!sg.inf) {
      g2j sj;
      g2j_from_aff(sj, sg);
      g2j_add(acc, acc, sj);
    }
  }
  if (bad) atomicOr(fail, 1);
  lds[lane] = acc;
  block_tree_reduce<g2j, 64>(lds, lane, g2j_add_op{});
  if (lane == 0 && !*fail) {
    g2a a;
    g2j_to_aff(a, lds[0]);
    // compress (ZCash): c1 || c0 big-endian, flags in byte 0
    if (a.inf) {
      for (int i = 0; i < 96; i++) out[i] = 0;
      out[0] = 0xC0;
    } else {
      fp_to_be48(a.x.c1, out);
      fp_to_be48(a.x.c0, out + 48);
      out[0] |= 0x80;
      if (fp2_gt_half_lex(a.y)) out[0] |= 0x20;
    }
  }
}

// one-thread test kernel: RFC 9380 h2c with an arbitrary DST, affine
// uncompressed output — pins the device sswu/iso/cofactor code against
// the literal RFC vectors (tests/golden/rfc9380_vectors.json)
__global__ void k_bls_h2c_dst(const uint8_t *__restrict__ msg,
                              uint32_t msg_len,
                              const uint8_t *__restrict__ dst,
                              uint32_t dst_len, uint8_t *__restrict__ out,
                              uint8_t *__restrict__ uni_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint8_t uni[256];
  expand_message_xmd_gen(msg, msg_len, dst, dst_len, 256, uni);
  for (int i = 0; i < 256; i++) uni_out[i] = uni[i];
  g2j h;
  h2c_g2_from_uniform(h, uni);
  g2a a;
  g2j_to_aff(a, h);
  g2_to_uncomp_dev(a, out);
}

// one-thread test kernel: a Jacobian G2 point as 192 uncompressed bytes
// (all zero for infinity, with *is_inf = 1)
__global__ void k_bls_g2j_uncomp(const g2j *__restrict__ p,
                                 uint8_t *__restrict__ out,
                                 int32_t *__restrict__ is_inf) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  g2a a;
  g2j_to_aff(a, p[0]);
  *is_inf = a.inf ? 1 : 0;
  if (a.inf) {
    for (int i = 0; i < 192; i++) out[i] = 0;
    return;
  }
  g2_to_uncomp_dev(a, out);
}

// test kernel, one lane per element: fp2_sqrt of a (c0 || c1, 48-byte
// big-endian each); ok[i] = 0 with out zeroed for a non-square or a
// non-canonical input
__global__ __launch_bounds__(64) void k_bls_fp2_sqrt_test(
    const uint8_t *__restrict__ in, uint64_t n, uint8_t *__restrict__ out,
    uint8_t *__restrict__ ok) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp2 a, r;
  fp2_zero(r);
  bool good = fp_from_be48(a.c0, in + 96 * i) &&
              fp_from_be48(a.c1, in + 96 * i + 48);
  if (good) good = fp2_sqrt(r, a);
  if (!good) fp2_zero(r);
  fp_to_be48(r.c0, out + 96 * i);
  fp_to_be48(r.c1, out + 96 * i + 48);
  ok[i] = good ? 1 : 0;
}

// test kernel, one lane per u (c0 || c1 big-endian): SSWU + isogeny +
// to-affine, no cofactor clear; 192 uncompressed bytes per point (all zero
// for a non-canonical u or a point at infinity). slow != 0 sends every u
// through sswu_g2_slow, the branch no ordinary input reaches.
__global__ __launch_bounds__(64) void k_bls_sswu_test(
    const uint8_t *__restrict__ in, uint64_t n, int slow,
    uint8_t *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp2 u;
  g2a q, a;
  a.inf = 1;
  if (fp_from_be48(u.c0, in + 96 * i) &&
      fp_from_be48(u.c1, in + 96 * i + 48)) {
    g2j pt;
    if (slow)
      sswu_g2_slow(q, u);
    else
      sswu_g2(q, u);
    iso_map_g2_j(pt, q);
    g2j_to_aff(a, pt);
  }
  if (a.inf) {
    for (int b = 0; b < 192; b++) out[192 * i + b] = 0;
    return;
  }
  g2_to_uncomp_dev(a, out + 192 * i);
}

// test kernel, one lane per point: w.h2c[i] as 192 uncompressed bytes
__global__ __launch_bounds__(64) void k_bls_h2c_uncomp_test(
    uint64_t n, BlsWork w, uint8_t *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2a a;
  g2j_to_aff(a, w.h2c[i]);
  if (a.inf) {
    for (int b = 0; b < 192; b++) out[192 * i + b] = 0;
    return;
  }
  g2_to_uncomp_dev(a, out + 192 * i);
}

// one-thread test kernel: general expand_message_xmd only
__global__ void k_bls_expand_dst(const uint8_t *__restrict__ msg,
                                 uint32_t msg_len,
                                 const uint8_t *__restrict__ dst,
                                 uint32_t dst_len, uint32_t len_in_bytes,
                                 uint8_t *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  expand_message_xmd_gen(msg, msg_len, dst, dst_len, len_in_bytes, out);
}

// ---- WAVE-SPLIT prepare, latency regime (n <= latency_max): the fused
// k_bls_prepare was one ~30 ms/lane serial kernel. Pass 1 decompresses
// sigma (n lanes; the sqrt pow chain dominates), pass 2 is the scalar-mult
// work in wave-uniform classes. Both take the full register budget (see
// k_bls_h2c_map_lat).
template <typename Fail>
__device__ __forceinline__ void sigdec_lane(const uint8_t *__restrict__ sigs,
                                            uint64_t n, const BlsWork &w,
                                            Fail fail) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2a sig;
  if (g2_decompress(sig, sigs + 96 * i) != 0) {
    fail.mark(i);
    sig.inf = 1; // harmless placeholder; the verdict is already forced false
  }
  g2j out;
  g2j_from_aff(out, sig);
  w.sig_aff[i] = out;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_bls_sigdec_lat(const uint8_t *__restrict__ sigs, uint64_t n,
                      BlsWork w) {
  sigdec_lane(sigs, n, w, BatchFail{w.fail});
}

// per-set twin: a signature that does not decode marks its own set
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_bls_sigdec_each(const uint8_t *__restrict__ sigs, uint64_t n,
                       BlsWork w, int32_t *__restrict__ status) {
  sigdec_lane(sigs, n, w, SetFail{status});
}

// THREE-class latency-regime mult pass (3n lanes): A [r]sigma,
// B [|x|]sigma + psi subgroup check, C [r]apk on G1. Every class is
// wave-uniform, no lane carries more than one chain, and the wave count
// is 3n/64 — a pure latency win for small and medium batches.
// The body runs the classes First..Last, n lanes each: A..C is the
// three-class kernel, B..C the two-class one that goes with the bucket MSM
// (which forms the sum of the [r_i]sigma_i without any of them), A alone
// the old signature sum of m3x_bls_sig_sum_test.
template <int First, int Last>
__device__ __forceinline__ void prep_mults_lane(
    const uint8_t *__restrict__ pks, const uint32_t *__restrict__ offs,
    const uint64_t *__restrict__ rands, uint64_t n, const BlsWork &w) {
  uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= (uint64_t)(Last - First + 1) * n) return;
  int cls = First + (lane < n ? 0 : (lane < 2 * n ? 1 : 2));
  uint64_t i = lane - (uint64_t)(cls - First) * n;
  if (First == 0 && cls == 0) { // A: rsig[i] = [r_i] sigma
    g2a sig;
    sig_aff_load(sig, w.sig_aff[i]);
    if (sig.inf) { // infinity contributes nothing to the signature sum
      g2j_set_inf(w.rsig[i]);
      return;
    }
    g2j rs;
    g2_mul_u64_aff(rs, sig, rands[i]);
    w.rsig[i] = rs;
    return;
  }
  if (Last >= 1 && cls == 1) { // B: deferred psi subgroup check (blst.rs:73-77)
    g2a sig;
    sig_aff_load(sig, w.sig_aff[i]);
    if (sig.inf) return; // infinity is a valid element
    g2j xsig_j;
    g2_mul_u64_aff(xsig_j, sig, BLS_X_ABS);
    if (!psi_eq_neg(sig, xsig_j)) atomicOr(w.fail, 1);
    return;
  }
  if (Last < 2) return;
  // C: p_scaled[i] = [r_i] apk
  uint32_t k0 = offs[i], k1 = offs[i + 1];
  if (k1 <= k0) {
    atomicOr(w.fail, 1);
    return;
  }
  g1j rp;
  if (k1 - k0 == 1) {
    g1a pk;
    if (g1_from_uncomp_trusted(pk, pks + 96 * (uint64_t)k0) != 0) {
      atomicOr(w.fail, 1);
      return;
    }
    if (pk.inf) {
      atomicOr(w.fail, 1);
      return;
    }
    g1_mul_u64_aff(rp, pk, rands[i]);
  } else {
    g1j apk = w.apk[i];
    if (g1j_is_inf(apk)) {
      atomicOr(w.fail, 1);
      return;
    }
    uint8_t rbe[8];
#pragma unroll
    for (int b = 0; b < 8; b++)
      rbe[b] = (uint8_t)(rands[i] >> (56 - 8 * b));
    g1j_mul_be_j(rp, apk, rbe, 8);
  }
  w.p_scaled[i] = rp;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_prep_mults3(const uint8_t *__restrict__ pks,
                       const uint32_t *__restrict__ offs,
                       const uint64_t *__restrict__ rands, uint64_t n,
                       BlsWork w) {
  prep_mults_lane<0, 2>(pks, offs, rands, n, w);
}

// classes B and C, 2n lanes: one full round of 2 waves/SIMD at 64k sets
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_prep_mults2(const uint8_t *__restrict__ pks,
                       const uint32_t *__restrict__ offs,
                       const uint64_t *__restrict__ rands, uint64_t n,
                       BlsWork w) {
  prep_mults_lane<1, 2>(pks, offs, rands, n, w);
}

// class A alone (m3x_bls_sig_sum_test's old path)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_prep_rsig(const uint64_t *__restrict__ rands, uint64_t n,
                     BlsWork w) {
  prep_mults_lane<0, 0>(nullptr, nullptr, rands, n, w);
}

// ---- per-set pipeline (m3x_bls_verify_each): SignatureSet::verify() for
// every set, generic_signature_set.rs:111-120 -> fast_aggregate_verify
// (blst.rs:250-261). Nothing is scaled by a randomiser: n independent
// equations e(apk_i, H(m_i)) * e(-g1, sigma_i) == 1 have nothing to
// batch, so classes A and C of k_bls_prep_mults3 have no counterpart.

// pass 2, n lanes: the deferred psi subgroup check (class B above) and the
// set's aggregate key. apk[i] is the parsed key lifted to Jacobian for
// k = 1 and k_bls_aggregate_w_each's sum for k > 1; a set without keys, or
// whose one key does not parse, leaves infinity there.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_prep_each(const uint8_t *__restrict__ pks,
                     const uint32_t *__restrict__ offs, uint64_t n, BlsWork w,
                     int32_t *__restrict__ status) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SetFail fail{status};
  uint32_t k0 = offs[i], k1 = offs[i + 1];
  if (k1 <= k0 || k1 - k0 == 1) {
    g1a pk;
    if (k1 <= k0 || g1_from_uncomp_trusted(pk, pks + 96 * (uint64_t)k0) != 0)
      pk.inf = 1; // placeholder
    g1j apk;
    g1j_from_aff(apk, pk);
    w.apk[i] = apk;
    if (pk.inf) fail.mark(i); // no key, unparsable key or infinity key
  } else if (g1j_is_inf(w.apk[i])) { // aggregate at infinity -> invalid
    fail.mark(i);
  }
  g2a sig;
  sig_aff_load(sig, w.sig_aff[i]);
  if (sig.inf) return; // infinity is a valid element (the equation fails)
  g2j xsig_j;
  g2_mul_u64_aff(xsig_j, sig, BLS_X_ABS);
  if (!psi_eq_neg(sig, xsig_j)) fail.mark(i);
}

// pass 3, the pairing check, is k_bls_verify_each in m3x_bls_each.hip: a
// translation unit of its own, so that a second caller of miller_w and
// final_exp_w here does not change how they inline into the batch tail.

// Above latency_max sets the kernels are issue-bound and the fused,
// default-register-budget forms win; at or below it the latency-regime
// forms do. Read per call (as M3X_SMALL_MILLER is) so a small test batch
// can be sent through the large-batch kernels.
uint64_t latency_max_sets() {
  if (const char *e = getenv("M3X_LATENCY_MAX")) return strtoull(e, nullptr, 10);
  return 1ull << 18;
}

// Smallest batch whose signature sum goes through the bucket MSM: below
// it the MSM's fixed bucket reduction costs more than class A's n chains
// save (DESIGN.md has the sweep). Read per call, as M3X_SMALL_MILLER is.
uint64_t sig_msm_min_sets() {
  if (const char *e = getenv("M3X_SIG_MSM_MIN")) return strtoull(e, nullptr, 10);
  return 4096;
}

void carve_sig_msm(m3x::ScratchCarver &c, BlsWork &w, uint64_t n) {
  w.msm.counts = c.take<uint32_t>(m3x::kSigMsmBuckets);
  w.msm.cursor = c.take<uint32_t>(m3x::kSigMsmBuckets);
  w.msm.idx = c.take<uint32_t>(m3x::kSigMsmWindows * n);
  w.msm.buckets = c.take<g2j>(m3x::kSigMsmBuckets);
  w.msm.win = c.take<g2j>(m3x::kSigMsmWindows);
}

// collect the k > 1 sets and sum their keys into w.apk; status == nullptr
// is the batch pipeline (w.fail), else the per-set one
void launch_aggregate(m3x_ctx *ctx, const void *pks_dev, const void *offs_dev,
                      uint64_t n, const BlsWork &w, int32_t *status) {
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  m3x::time_begin(ctx, M3X_K_BLS_AGG);
  hipLaunchKernelGGL(k_bls_scan_agg, dim3(blocks), dim3(64), 0, ctx->stream,
                     (const uint32_t *)offs_dev, n, w);
  uint32_t agg_blocks = n < kAggMaxBlocks ? (uint32_t)n : kAggMaxBlocks;
  if (status)
    hipLaunchKernelGGL(k_bls_aggregate_w_each, dim3(agg_blocks), dim3(64), 0,
                       ctx->stream, (const uint8_t *)pks_dev,
                       (const uint32_t *)offs_dev, w, status);
  else
    hipLaunchKernelGGL(k_bls_aggregate_w, dim3(agg_blocks), dim3(64), 0,
                       ctx->stream, (const uint8_t *)pks_dev,
                       (const uint32_t *)offs_dev, w);
  m3x::time_end(ctx, M3X_K_BLS_AGG);
}

// w.h2c[i] = hash_to_curve(msg_i) on the second stream (h2c needs nothing
// from the prepare kernels, so the two ~1-wave/SIMD chains co-reside), and
// the main stream's wait for it
int launch_h2c(m3x_ctx *ctx, const void *msgs_dev, uint64_t n,
               uint64_t latency_max, const BlsWork &w) {
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  m3x::time_begin_s(ctx, M3X_K_BLS_H2C, ctx->stream2);
  if (n > 64) { // split h2c pays at small n too (per-lane chain is ONE
                // point, then the clear, vs two points + clear in the fused
                // form)
    uint32_t blocks2 = (uint32_t)((2 * n + 63) / 64);
    hipLaunchKernelGGL(k_bls_h2c_expand, dim3(blocks), dim3(64), 0,
                       ctx->stream2, (const uint8_t *)msgs_dev, n, w);
    if (n <= latency_max) {
      hipLaunchKernelGGL(k_bls_h2c_map_lat, dim3(blocks2), dim3(64), 0,
                         ctx->stream2, n, w);
      hipLaunchKernelGGL(k_bls_h2c_fin_lat, dim3(blocks), dim3(64), 0,
                         ctx->stream2, n, w);
    } else {
      hipLaunchKernelGGL(k_bls_h2c_map, dim3(blocks2), dim3(64), 0,
                         ctx->stream2, n, w);
      hipLaunchKernelGGL(k_bls_h2c_fin, dim3(blocks), dim3(64), 0,
                         ctx->stream2, n, w);
    }
  } else {
    hipLaunchKernelGGL(k_bls_h2c, dim3(blocks), dim3(64), 0, ctx->stream2,
                       (const uint8_t *)msgs_dev, n, w);
  }
  m3x::time_end_s(ctx, M3X_K_BLS_H2C, ctx->stream2);
  M3X_HIP_CHECK(hipEventRecord(ctx->ev_s2, ctx->stream2));
  M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_s2, 0));
  return M3X_OK;
}

// The per-set pipeline. It shares scratch_a with run_verify under a layout
// of its own; each call zeroes what it reads before writing (status,
// agg_count), as run_verify does (fail, agg_count), and both end with the
// main stream synchronised after it has joined the h2c stream, so neither
// leaves anything behind for the other. No reductions and no side stream:
// a verdict belongs to a set.
int run_each(m3x_ctx *ctx, const void *msgs_dev, const void *sigs_dev,
             const void *pks_dev, const void *offs_dev, uint64_t n,
             int32_t *verdicts_dev) {
  BlsWork w = {};
  int32_t *status = nullptr;
  int rc = m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.apk = c.take<g1j>(n);
        w.agg_idx = c.take<uint64_t>(n);
        w.agg_count = c.take<uint32_t>(1);
        w.h2c = c.take<g2j>(n);
        w.uni = c.take<uint8_t>(n * 256);
        w.h2c_pts = c.take<g2j>(2 * n);
        w.sig_aff = c.take<g2j>(n);
        status = c.take<int32_t>(n);
      });
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(status, 0, 4 * n, ctx->stream));
  M3X_HIP_CHECK(hipMemsetAsync(w.agg_count, 0, 4, ctx->stream));
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  launch_aggregate(ctx, pks_dev, offs_dev, n, w, status);
  m3x::time_begin(ctx, M3X_K_BLS_PREPARE);
  hipLaunchKernelGGL(k_bls_sigdec_each, dim3(blocks), dim3(64), 0, ctx->stream,
                     (const uint8_t *)sigs_dev, n, w, status);
  hipLaunchKernelGGL(k_bls_prep_each, dim3(blocks), dim3(64), 0, ctx->stream,
                     (const uint8_t *)pks_dev, (const uint32_t *)offs_dev, n,
                     w, status);
  m3x::time_end(ctx, M3X_K_BLS_PREPARE);
  DBG_STEP(ctx, "each prepare");
  rc = launch_h2c(ctx, msgs_dev, n, latency_max_sets(), w);
  if (rc != M3X_OK) return rc;
  DBG_STEP(ctx, "each h2c");
  m3x::time_begin(ctx, M3X_K_BLS_EACH);
  m3x::launch_bls_verify_each(ctx->stream, n, w.apk, w.h2c, w.sig_aff, status,
                              verdicts_dev);
  m3x::time_end(ctx, M3X_K_BLS_EACH);
  DBG_STEP(ctx, "each verify");
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return M3X_OK;
}

int run_verify(m3x_ctx *ctx, const void *msgs_dev, const void *sigs_dev,
               const void *pks_dev, const void *offs_dev,
               const void *rands_dev, uint64_t n, int32_t *out) {
  BlsWork w;
  uint64_t latency_max = latency_max_sets();
  // the signature sum as a bucket MSM on the side stream (latency regime
  // only: the fused k_bls_prepare shares sigma's doubling chain between
  // [r]sigma and the subgroup check, so there the sum is not a class apart)
  bool use_msm = n <= latency_max && n >= sig_msm_min_sets() &&
                 n <= m3x::kSigMsmMaxSets;
  int rc = m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.apk = c.take<g1j>(n);
        w.agg_idx = c.take<uint64_t>(n);
        w.agg_count = c.take<uint32_t>(1);
        w.p_scaled = c.take<g1j>(n);
        w.h2c = c.take<g2j>(n);
        w.uni = c.take<uint8_t>(n * 256);
        w.h2c_pts = c.take<g2j>(2 * n);
        w.rsig = c.take<g2j>(n);
        w.sig_aff = c.take<g2j>(n);
        w.fparts = c.take<fp12m>(2 * n); // split miller: 2n partials
        w.fail = c.take<int>(1);
        w.sig_stage = c.take<g2j>(kReduceMaxBlocks);
        w.sig_sum = c.take<g2j>(1);
        w.gt_stage = c.take<fp12m>(kReduceMaxBlocks);
        w.gt_parts = c.take<fp12m>(1);
        w.sig_gt = c.take<fp12m>(1);
        w.verdict = c.take<int>(1);
        if (use_msm) carve_sig_msm(c, w, n);
      });
  if (rc != M3X_OK) return rc;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  M3X_HIP_CHECK(hipMemsetAsync(w.agg_count, 0, 4, ctx->stream));
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  launch_aggregate(ctx, pks_dev, offs_dev, n, w, nullptr);
  m3x::time_begin(ctx, M3X_K_BLS_PREPARE);
  if (n > latency_max) {
    // issue-bound regime: the fused shared-chain kernel does less work
    hipLaunchKernelGGL(k_bls_prepare, dim3(blocks), dim3(64), 0,
                       ctx->stream, (const uint8_t *)sigs_dev,
                       (const uint8_t *)pks_dev, (const uint32_t *)offs_dev,
                       (const uint64_t *)rands_dev, n, w);
  } else {
    // latency regime: decompress pass + two wave-uniform mult classes,
    // full-register-budget twins
    hipLaunchKernelGGL(k_bls_sigdec_lat, dim3(blocks), dim3(64), 0,
                       ctx->stream, (const uint8_t *)sigs_dev, n, w);
    if (use_msm) {
      // sig_aff is complete: release the MSM, which then shares the GPU
      // with classes B and C and with h2c
      M3X_HIP_CHECK(hipEventRecord(ctx->ev_pipe[2], ctx->stream));
      uint32_t blocks2 = (uint32_t)((2 * n + 63) / 64);
      hipLaunchKernelGGL(k_bls_prep_mults2, dim3(blocks2), dim3(64), 0,
                         ctx->stream, (const uint8_t *)pks_dev,
                         (const uint32_t *)offs_dev,
                         (const uint64_t *)rands_dev, n, w);
    } else {
      uint32_t blocks3 = (uint32_t)((3 * n + 63) / 64);
      hipLaunchKernelGGL(k_bls_prep_mults3, dim3(blocks3), dim3(64), 0,
                         ctx->stream, (const uint8_t *)pks_dev,
                         (const uint32_t *)offs_dev,
                         (const uint64_t *)rands_dev, n, w);
    }
  }
  m3x::time_end(ctx, M3X_K_BLS_PREPARE);
  if (use_msm) {
    M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream3, ctx->ev_pipe[2], 0));
    m3x::time_begin_s(ctx, M3X_K_BLS_SIGMSM, ctx->stream3);
    rc = m3x::launch_bls_sig_msm(ctx->stream3, n, w.sig_aff,
                                 (const uint64_t *)rands_dev, w.msm,
                                 w.sig_sum);
    if (rc != M3X_OK) return rc;
    m3x::time_end_s(ctx, M3X_K_BLS_SIGMSM, ctx->stream3);
  }
  DBG_STEP(ctx, "prepare");
  // h2c is independent of prepare: run it on the second stream so the two
  // ~1-wave/SIMD kernels co-reside (both fit at 2 waves/SIMD by VGPR count)
  rc = launch_h2c(ctx, msgs_dev, n, latency_max, w);
  if (rc != M3X_OK) return rc;
  DBG_STEP(ctx, "h2c");
  m3x::time_begin(ctx, M3X_K_BLS_MILLER);
  // small batches are latency-bound on the per-lane kernel: go wave-per-set
  uint64_t small_thresh = 2048; // measured crossover (tmp_bench/c4probe)
  if (const char *e = getenv("M3X_SMALL_MILLER")) small_thresh = strtoull(e, nullptr, 10);
  uint64_t n_parts = n; // fp12 partials feeding the GT reduce
  // read per call (as M3X_SMALL_MILLER is) so both forms are testable
  // in-process; measured SLOWER at C2 (57 vs 44 ms: the 256-VGPR cap
  // spills more than co-residency saves)
  const char *split_env = getenv("M3X_MILLER_SPLIT");
  bool use_split = split_env && split_env[0] == '1';
  if (n <= small_thresh) {
    hipLaunchKernelGGL(k_bls_miller_small, dim3((uint32_t)n), dim3(64), 0,
                       ctx->stream, n, w);
  } else if (use_split) {
    n_parts = 2 * n; // wave-split: two half-Millers per set
    uint32_t blocks2 = (uint32_t)((2 * n + 63) / 64);
    hipLaunchKernelGGL(k_bls_miller_split, dim3(blocks2), dim3(64), 0,
                       ctx->stream, n, w);
  } else {
    hipLaunchKernelGGL(k_bls_miller, dim3(blocks), dim3(64), 0, ctx->stream,
                       n, w);
  }
  m3x::time_end(ctx, M3X_K_BLS_MILLER);
  DBG_STEP(ctx, "miller");
  // The batch tail is two independent chains:
  //   main stream : reduce_gt x2                        -> gt_parts
  //   stream3     : [reduce_sig x2 ->] sigpair (Miller) -> sig_gt
  // joined by k_bls_finish. stream3 is the sole writer of sig_stage,
  // sig_sum and sig_gt; nothing else touches them until k_bls_finish,
  // which waits on ev_pipe[1]. With the MSM path sig_sum is already there:
  // the MSM ran on stream3 behind ev_pipe[2] (recorded after
  // k_bls_sigdec_lat, the last writer of sig_aff, its only input besides
  // rands), and stream order puts k_bls_sigpair after it. Otherwise
  // reduce_sig x2 form it here from rsig (complete once the prepare
  // kernels are). Either way the pairing is released after the per-set
  // Miller kernel. Releasing it right after the prepare kernels was measured and
  // gains nothing: prepare, not h2c, is what the Miller kernel waits for,
  // so the chain then starts together with that kernel, which owns every
  // SIMD's register file — reduce_sig starves and the Miller kernel grows
  // by what the tail saves ("Tail placement").
  // The next call on this context cannot overtake the side
  // stream: the verdict read-back below synchronises the main stream,
  // whose k_bls_finish has by then waited for the side stream's last
  // kernel.
  // M3X_SIGPAIR_EARLY=1 (read per call; MSM path only) drops that wait, so
  // the pairing follows the MSM at once: the measured alternative.
  const char *early_env = getenv("M3X_SIGPAIR_EARLY");
  if (!(use_msm && early_env && early_env[0] == '1')) {
    M3X_HIP_CHECK(hipEventRecord(ctx->ev_pipe[0], ctx->stream));
    M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream3, ctx->ev_pipe[0], 0));
  }
  uint32_t sblocks = (uint32_t)((n + kReduceThreads - 1) / kReduceThreads);
  if (sblocks > kReduceMaxBlocks) sblocks = kReduceMaxBlocks;
  m3x::time_begin_s(ctx, M3X_K_BLS_SIGPAIR, ctx->stream3);
  if (!use_msm) {
    hipLaunchKernelGGL(k_bls_reduce_sig, dim3(sblocks), dim3(kReduceThreads),
                       0, ctx->stream3, w.rsig, n, w.sig_stage);
    hipLaunchKernelGGL(k_bls_reduce_sig, dim3(1), dim3(kReduceThreads), 0,
                       ctx->stream3, w.sig_stage, (uint64_t)sblocks,
                       w.sig_sum);
  }
  hipLaunchKernelGGL(k_bls_sigpair, dim3(1), dim3(64), 0, ctx->stream3, w);
  m3x::time_end_s(ctx, M3X_K_BLS_SIGPAIR, ctx->stream3);
  M3X_HIP_CHECK(hipEventRecord(ctx->ev_pipe[1], ctx->stream3));
  uint32_t rblocks =
      (uint32_t)((n_parts + kReduceThreads - 1) / kReduceThreads);
  if (rblocks > kReduceMaxBlocks) rblocks = kReduceMaxBlocks;
  m3x::time_begin(ctx, M3X_K_BLS_REDUCE);
  hipLaunchKernelGGL(k_bls_reduce_gt, dim3(rblocks), dim3(kReduceThreads), 0,
                     ctx->stream, w.fparts, n_parts, w.gt_stage);
  hipLaunchKernelGGL(k_bls_reduce_gt, dim3(1), dim3(kReduceThreads), 0,
                     ctx->stream, w.gt_stage, (uint64_t)rblocks, w.gt_parts);
  m3x::time_end(ctx, M3X_K_BLS_REDUCE);
  DBG_STEP(ctx, "reduce");
  M3X_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_pipe[1], 0));
  m3x::time_begin(ctx, M3X_K_BLS_FINISH);
  hipLaunchKernelGGL(k_bls_finish, dim3(1), dim3(64), 0, ctx->stream, w);
  m3x::time_end(ctx, M3X_K_BLS_FINISH);
  DBG_STEP(ctx, "finish");
  int32_t verdict = 0;
  M3X_HIP_CHECK(hipMemcpyAsync(&verdict, w.verdict, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
  M3X_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = verdict;
  return M3X_OK;
}

} // namespace

extern "C" {

int32_t m3x_bls_pk_decompress(m3x_ctx *ctx, const uint8_t *comp, uint64_t n,
                              uint8_t *uncomp, int32_t *status) {
  if (!ctx || n == 0) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *comp_d = tmp.upload(comp, n * 48);
  uint8_t *unc_d = tmp.alloc(n * 96);
  int32_t *st_d = tmp.alloc<int32_t>(n * 4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  hipLaunchKernelGGL(k_bls_pk_decompress, dim3(blocks), dim3(64), 0,
                     ctx->stream, comp_d, n, unc_d, st_d);
  tmp.download(uncomp, unc_d, n * 96);
  tmp.download(status, st_d, n * 4);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_bls_expand_test(m3x_ctx *ctx, const uint8_t *msg,
                            uint32_t msg_len, const uint8_t *dst,
                            uint32_t dst_len, uint32_t len_in_bytes,
                            uint8_t *out) {
  if (!ctx || msg_len > 544 || dst_len == 0 || dst_len > 255 ||
      len_in_bytes > 256)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *msg_d = tmp.upload(msg, msg_len);
  const uint8_t *dst_d = tmp.upload(dst, dst_len);
  uint8_t *out_d = tmp.alloc(256);
  if (!tmp.ok()) return M3X_ERR_HIP;
  hipLaunchKernelGGL(k_bls_expand_dst, dim3(1), dim3(1), 0, ctx->stream,
                     msg_d, msg_len, dst_d, dst_len, len_in_bytes, out_d);
  tmp.download(out, out_d, len_in_bytes);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_bls_h2c_test(m3x_ctx *ctx, const uint8_t *msg, uint32_t msg_len,
                         const uint8_t *dst, uint32_t dst_len,
                         uint8_t out_uncomp[192], uint8_t out_uniform[256]) {
  if (!ctx || msg_len > 544 || dst_len == 0 || dst_len > 255)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *msg_d = tmp.upload(msg, msg_len);
  const uint8_t *dst_d = tmp.upload(dst, dst_len);
  uint8_t *pt_d = tmp.alloc(192), *uni_d = tmp.alloc(256);
  if (!tmp.ok()) return M3X_ERR_HIP;
  hipLaunchKernelGGL(k_bls_h2c_dst, dim3(1), dim3(1), 0, ctx->stream, msg_d,
                     msg_len, dst_d, dst_len, pt_d, uni_d);
  tmp.download(out_uncomp, pt_d, 192);
  if (out_uniform) tmp.download(out_uniform, uni_d, 256);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_bls_fp2_sqrt_test(m3x_ctx *ctx, const uint8_t *a, uint64_t n,
                              uint8_t *out, uint8_t *ok) {
  if (!ctx || !a || !out || !ok || n == 0 || n > (1u << 20))
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *a_d = tmp.upload(a, n * 96);
  uint8_t *out_d = tmp.alloc(n * 96), *ok_d = tmp.alloc(n);
  if (!tmp.ok()) return M3X_ERR_HIP;
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  hipLaunchKernelGGL(k_bls_fp2_sqrt_test, dim3(blocks), dim3(64), 0,
                     ctx->stream, a_d, n, out_d, ok_d);
  tmp.download(out, out_d, n * 96);
  tmp.download(ok, ok_d, n);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

static int32_t sswu_test(m3x_ctx *ctx, const uint8_t *u, uint64_t n, int slow,
                         uint8_t *out) {
  if (!ctx || !u || !out || n == 0 || n > (1u << 20)) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *u_d = tmp.upload(u, n * 96);
  uint8_t *out_d = tmp.alloc(n * 192);
  if (!tmp.ok()) return M3X_ERR_HIP;
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  hipLaunchKernelGGL(k_bls_sswu_test, dim3(blocks), dim3(64), 0, ctx->stream,
                     u_d, n, slow, out_d);
  tmp.download(out, out_d, n * 192);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_bls_sswu_test(m3x_ctx *ctx, const uint8_t *u, uint64_t n,
                          uint8_t *out) {
  return sswu_test(ctx, u, n, 0, out);
}

int32_t m3x_bls_sswu_slow_test(m3x_ctx *ctx, const uint8_t *u, uint64_t n,
                               uint8_t *out) {
  return sswu_test(ctx, u, n, 1, out);
}

int32_t m3x_bls_h2c_batch_test(m3x_ctx *ctx, const uint8_t *msgs, uint64_t n,
                               int32_t mode, uint8_t *out) {
  if (!ctx || !msgs || !out || n == 0 || n > (1u << 20) || mode < 0 ||
      mode > 2)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  BlsWork w = {};
  uint8_t *out_d = nullptr;
  int rc = m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.h2c = c.take<g2j>(n);
        w.uni = c.take<uint8_t>(n * 256);
        w.h2c_pts = c.take<g2j>(2 * n);
        out_d = c.take<uint8_t>(n * 192);
      });
  if (rc != M3X_OK) return rc;
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *msgs_d = tmp.upload(msgs, n * 32);
  if (!tmp.ok()) return M3X_ERR_HIP;
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  uint32_t blocks2 = (uint32_t)((2 * n + 63) / 64);
  if (mode == 0) {
    hipLaunchKernelGGL(k_bls_h2c, dim3(blocks), dim3(64), 0, ctx->stream,
                       msgs_d, n, w);
  } else {
    hipLaunchKernelGGL(k_bls_h2c_expand, dim3(blocks), dim3(64), 0,
                       ctx->stream, msgs_d, n, w);
    if (mode == 1) {
      hipLaunchKernelGGL(k_bls_h2c_map, dim3(blocks2), dim3(64), 0,
                         ctx->stream, n, w);
      hipLaunchKernelGGL(k_bls_h2c_fin, dim3(blocks), dim3(64), 0,
                         ctx->stream, n, w);
    } else {
      hipLaunchKernelGGL(k_bls_h2c_map_lat, dim3(blocks2), dim3(64), 0,
                         ctx->stream, n, w);
      hipLaunchKernelGGL(k_bls_h2c_fin_lat, dim3(blocks), dim3(64), 0,
                         ctx->stream, n, w);
    }
  }
  hipLaunchKernelGGL(k_bls_h2c_uncomp_test, dim3(blocks), dim3(64), 0,
                     ctx->stream, n, w, out_d);
  tmp.download(out, out_d, n * 192);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

int32_t m3x_bls_sig_sum_test(m3x_ctx *ctx, const uint8_t *sigs,
                             const uint64_t *rands, uint64_t n,
                             int32_t use_msm, uint8_t out_uncomp[192]) {
  if (!ctx || !sigs || !rands || !out_uncomp || n == 0 ||
      n > m3x::kSigMsmMaxSets)
    return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  BlsWork w = {};
  int32_t *is_inf = nullptr;
  uint8_t *out_d = nullptr;
  int rc = m3x::carve_scratch(
      ctx, &ctx->scratch_a, &ctx->scratch_a_bytes, [&](m3x::ScratchCarver &c) {
        w.rsig = c.take<g2j>(n);
        w.sig_aff = c.take<g2j>(n);
        w.fail = c.take<int>(1);
        w.sig_stage = c.take<g2j>(kReduceMaxBlocks);
        w.sig_sum = c.take<g2j>(1);
        is_inf = c.take<int32_t>(1);
        out_d = c.take<uint8_t>(192);
        carve_sig_msm(c, w, n);
      });
  if (rc != M3X_OK) return rc;
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *sigs_d = tmp.upload(sigs, n * 96);
  const uint64_t *rands_d = tmp.upload(rands, n * 8);
  if (!tmp.ok()) return M3X_ERR_HIP;
  M3X_HIP_CHECK(hipMemsetAsync(w.fail, 0, 4, ctx->stream));
  uint32_t blocks = (uint32_t)((n + 63) / 64);
  hipLaunchKernelGGL(k_bls_sigdec_lat, dim3(blocks), dim3(64), 0, ctx->stream,
                     sigs_d, n, w);
  if (use_msm) {
    rc = m3x::launch_bls_sig_msm(ctx->stream, n, w.sig_aff, rands_d, w.msm,
                                 w.sig_sum);
    if (rc != M3X_OK) {
      (void)tmp.sync();
      return rc;
    }
  } else {
    hipLaunchKernelGGL(k_bls_prep_rsig, dim3(blocks), dim3(64), 0, ctx->stream,
                       rands_d, n, w);
    uint32_t sblocks = (uint32_t)((n + kReduceThreads - 1) / kReduceThreads);
    if (sblocks > kReduceMaxBlocks) sblocks = kReduceMaxBlocks;
    hipLaunchKernelGGL(k_bls_reduce_sig, dim3(sblocks), dim3(kReduceThreads),
                       0, ctx->stream, w.rsig, n, w.sig_stage);
    hipLaunchKernelGGL(k_bls_reduce_sig, dim3(1), dim3(kReduceThreads), 0,
                       ctx->stream, w.sig_stage, (uint64_t)sblocks, w.sig_sum);
  }
  hipLaunchKernelGGL(k_bls_g2j_uncomp, dim3(1), dim3(1), 0, ctx->stream,
                     w.sig_sum, out_d, is_inf);
  int32_t fail = 1, inf = 0;
  tmp.download(out_uncomp, out_d, 192);
  tmp.download(&fail, w.fail, 4);
  tmp.download(&inf, is_inf, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  if (fail) return M3X_ERR_ENCODING;
  return inf ? 1 : 0;
}

int32_t m3x_bls_sig_aggregate(m3x_ctx *ctx, const uint8_t *sigs, uint64_t n,
                              uint8_t out_sig[96]) {
  if (!ctx || n == 0) return M3X_ERR_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *sigs_d = tmp.upload(sigs, n * 96);
  uint8_t *out_d = tmp.alloc(96);
  int *fail_d = tmp.alloc<int>(4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  M3X_HIP_CHECK(hipMemsetAsync(fail_d, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_bls_sig_aggregate_w, dim3(1), dim3(64), 0, ctx->stream,
                     sigs_d, n, out_d, fail_d);
  int fail = 1;
  tmp.download(out_sig, out_d, 96);
  tmp.download(&fail, fail_d, 4);
  if (!tmp.sync()) return M3X_ERR_HIP;
  return fail ? M3X_ERR_ARG : M3X_OK;
}

int32_t m3x_bls_verify_sets_dev(m3x_ctx *ctx, const void *msgs_dev,
                                const void *sigs_dev, const void *pks_dev,
                                const void *pk_offsets_dev,
                                const void *rands_dev, uint64_t n) {
  if (!ctx) return M3X_ERR_ARG;
  if (n == 0) return 0; // blst.rs:42-44 (host normally short-circuits)
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  int32_t verdict = 0;
  int rc = run_verify(ctx, msgs_dev, sigs_dev, pks_dev, pk_offsets_dev,
                      rands_dev, n, &verdict);
  if (rc != M3X_OK) return rc;
  return verdict;
}

int32_t m3x_bls_verify_sets(m3x_ctx *ctx, const uint8_t *msgs,
                            const uint8_t *sigs, const uint8_t *pks,
                            const uint32_t *pk_offsets, const uint64_t *rands,
                            uint64_t n) {
  if (!ctx) return M3X_ERR_ARG;
  if (n == 0) return 0;
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint64_t nk = pk_offsets[n];
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *msgs_d = tmp.upload(msgs, n * 32);
  const uint8_t *sigs_d = tmp.upload(sigs, n * 96);
  const uint8_t *pks_d = tmp.upload(pks, nk * 96);
  const uint32_t *offs_d = tmp.upload(pk_offsets, (n + 1) * 4);
  const uint64_t *rands_d = tmp.upload(rands, n * 8);
  if (!tmp.ok()) return M3X_ERR_HIP;
  return m3x_bls_verify_sets_dev(ctx, msgs_d, sigs_d, pks_d, offs_d, rands_d,
                                 n);
}

int32_t m3x_bls_verify_each_dev(m3x_ctx *ctx, const void *msgs_dev,
                                const void *sigs_dev, const void *pks_dev,
                                const void *pk_offsets_dev, uint64_t n,
                                void *verdicts_dev) {
  // one block per set: n is a grid dimension
  if (!ctx || n > 0x7fffffffull) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  return run_each(ctx, msgs_dev, sigs_dev, pks_dev, pk_offsets_dev, n,
                  (int32_t *)verdicts_dev);
}

int32_t m3x_bls_verify_each(m3x_ctx *ctx, const uint8_t *msgs,
                            const uint8_t *sigs, const uint8_t *pks,
                            const uint32_t *pk_offsets, uint64_t n,
                            int32_t *verdicts) {
  if (!ctx || n > 0x7fffffffull) return M3X_ERR_ARG;
  if (n == 0) return M3X_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  M3X_HIP_CHECK(hipSetDevice(ctx->device));
  uint64_t nk = pk_offsets[n];
  m3x::DevTemps tmp(ctx->stream);
  const uint8_t *msgs_d = tmp.upload(msgs, n * 32);
  const uint8_t *sigs_d = tmp.upload(sigs, n * 96);
  const uint8_t *pks_d = tmp.upload(pks, nk * 96);
  const uint32_t *offs_d = tmp.upload(pk_offsets, (n + 1) * 4);
  int32_t *verdicts_d = tmp.alloc<int32_t>(n * 4);
  if (!tmp.ok()) return M3X_ERR_HIP;
  int rc = m3x_bls_verify_each_dev(ctx, msgs_d, sigs_d, pks_d, offs_d, n,
                                   verdicts_d);
  if (rc != M3X_OK) return rc;
  tmp.download(verdicts, verdicts_d, n * 4);
  return tmp.sync() ? M3X_OK : M3X_ERR_HIP;
}

} // extern "C"
