// Shared context for the m3x_consensus library (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

// named kernel slots for per-kernel HIP-event timing (m3x_kernel_ms)
enum m3x_kernel_id {
  M3X_K_LEAVES = 0,
  M3X_K_REDUCE = 1,
  M3X_K_FINALIZE = 2,
  M3X_K_BLS_PREPARE = 3,
  M3X_K_BLS_H2C = 4,
  M3X_K_BLS_MILLER = 5,
  M3X_K_BLS_REDUCE = 6,
  M3X_K_BLS_FINISH = 7,
  M3X_K_BLS_AGG = 8,
  M3X_K_KZG_CHALLENGE = 9, // per-blob Fiat-Shamir hash (stream2)
  M3X_K_KZG_DECOMP = 10,   // commitment/proof decompress + subgroup check
  M3X_K_KZG_EVAL = 11,     // blob evaluation at z
  M3X_K_KZG_BATCH_R = 12,  // batch challenge + scalar powers
  M3X_K_KZG_MULTS = 13,    // G1 scalar multiplications
  M3X_K_KZG_REDUCE = 14,   // G1 sums
  M3X_K_KZG_FINISH = 15,   // pairing check
  M3X_K_KZGP_QUOTIENT = 16, // proof quotient in evaluation form
  M3X_K_KZGP_MSM = 17,      // fixed-base MSM: table look-ups + block sums
  M3X_K_KZGP_FINISH = 18,   // last G1 sum + compression
  M3X_K_BLS_SIGPAIR = 19,   // signature pairing (stream3); with the old
                            // path also the signature sum before it
  M3X_K_BLS_EACH = 20,      // per-set pairing check (m3x_bls_verify_each)
  M3X_K_KZGC_NTT = 21,      // compute_cells: the three transform passes
  M3X_K_KZGC_DECODE = 22,   // cell evaluations: canonical check + decode
  M3X_K_KZGC_COMBINE = 23,  // r powers, row weights, column interpolation
  M3X_K_KZGC_RECOVER = 24,  // recover_cells: vanishing values + five passes
  // 25 is not a slot: it was the first id past the table when the table
  // had 25 entries, callers probe it as such (tests/test_gpu_kzg_recover.py
  // does), and m3x_kernel_ms keeps answering M3X_ERR_ARG for it
  M3X_K_RESERVED_25 = 25,
  M3X_K_BLS_SIGMSM = 26,    // signature sum by bucket MSM (stream3)
  M3X_K_KZGC_TOEPLITZ = 27,  // cell proofs: coefficient pass + Toeplitz sums
  M3X_K_KZGC_PROOF_DFT = 28, // cell proofs: 128-point G1 transform + compress
  M3X_K_COUNT = 29
};

struct m3x_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr; // overlap of independent kernels
  hipStream_t stream3 = nullptr; // third pipeline stage
  hipEvent_t ev_s2 = nullptr;
  hipEvent_t ev_pipe[24] = {};   // chunk-pipeline dependencies
  // device-resident zero-hash ladder Z[0..64] (computed on GPU at create)
  uint8_t *zeros_dev = nullptr;
  // growable scratch buffers for merkle reduction stages
  uint8_t *scratch_a = nullptr;
  uint64_t scratch_a_bytes = 0;
  uint8_t *scratch_b = nullptr;
  uint64_t scratch_b_bytes = 0;
  // persistent pool for small inputs + 32B root slots (avoids per-call
  // hipMalloc/hipFree on the many tiny container merkleizations)
  uint8_t *small_pool = nullptr; // layout: [256 KiB input][64B root]
  // The root slot at small_pool + SMALL_POOL_IN is [32B result][32B
  // intermediate], shared by every merkle call that ends in a root copy-back
  // (chunks, validator subtree / registry, registry cache); pooled inputs and
  // finalize_root's node stay below SMALL_POOL_IN. All of them hold `mu` and
  // run on `stream`, so stream order is the only ordering the slot needs.
  static constexpr uint64_t SMALL_POOL_IN = 256 * 1024;
  // per-kernel cumulative time (ms) + launch counts since last reset,
  // measured with hipEvents on `stream`
  hipEvent_t ev_a[M3X_K_COUNT] = {};
  hipEvent_t ev_b[M3X_K_COUNT] = {};
  double kernel_ms[M3X_K_COUNT] = {};
  uint64_t kernel_launches[M3X_K_COUNT] = {};
  bool timing = false;
  std::recursive_mutex mu; // one context serializes its own calls
};

namespace m3x {
// wrap a launch with events when ctx->timing (call after the launch)
void time_begin(m3x_ctx *ctx, int k);
void time_end(m3x_ctx *ctx, int k);
void time_begin_s(m3x_ctx *ctx, int k, hipStream_t st);
void time_end_s(m3x_ctx *ctx, int k, hipStream_t st);
} // namespace m3x

#define M3X_HIP_CHECK(expr)                                                    \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) return M3X_ERR_HIP;                                  \
  } while (0)

namespace m3xb {
struct g1j;
struct g2j;
} // namespace m3xb

namespace m3x {
// m3x_bls_each.hip: the per-set pairing kernel of m3x_bls_verify_each, one
// wave per set, over the arrays the stages in m3x_bls.hip left behind;
// verdicts[i] = 1/0, forced to 0 where status[i] != 0
void launch_bls_verify_each(hipStream_t st, uint64_t n, const m3xb::g1j *apk,
                            const m3xb::g2j *h2c, const m3xb::g2j *sig_aff,
                            const int32_t *status, int32_t *verdicts);

// m3x_bls_msm.hip: sig_sum[0] = sum r_i * sigma_i by a bucket MSM over
// unsigned windows of the 64-bit r_i. The window width is this one
// constant; everything else follows from it.
constexpr int kSigMsmWindowBits = 8;
constexpr int kSigMsmWindows = (64 + kSigMsmWindowBits - 1) / kSigMsmWindowBits;
constexpr int kSigMsmDigits = 1 << kSigMsmWindowBits; // digit 0 is skipped
constexpr int kSigMsmBuckets = kSigMsmWindows * kSigMsmDigits;
// largest batch the MSM takes: positions in idx are 32-bit
constexpr uint64_t kSigMsmMaxSets = (1ull << 32) / kSigMsmWindows - 1;
struct SigMsmWork {
  uint32_t *counts;      // [kSigMsmBuckets] entries per (window, digit)
  uint32_t *cursor;      // [kSigMsmBuckets] start of each bucket in idx, then
                         // the scatter's write position
  uint32_t *idx;         // [kSigMsmWindows * n] set indices, sorted by bucket
  m3xb::g2j *buckets;    // [kSigMsmBuckets] bucket sums
  m3xb::g2j *win;        // [kSigMsmWindows] [2^(c*w)] * window sum
};
// sig_aff as k_bls_sigdec_lat leaves it (z = 1 affine, z = 0 infinity);
// every launch, and the zeroing of counts, goes on st. Returns 0 or
// M3X_ERR_HIP.
int launch_bls_sig_msm(hipStream_t st, uint64_t n, const m3xb::g2j *sig_aff,
                       const uint64_t *rands, const SigMsmWork &m,
                       m3xb::g2j *sig_sum);

// ensure scratch buffer has at least `bytes`; returns 0 or M3X_ERR_*
int ensure_scratch(m3x_ctx *ctx, uint8_t **buf, uint64_t *cur, uint64_t bytes);

// Carves one scratch buffer into 256-byte-aligned pieces. A layout is
// written once, as a function of the carver: with a null base take() only
// advances the offset (sizing pass), over the real buffer it returns the
// pointers.
struct ScratchCarver {
  uint8_t *base;
  uint64_t off = 0;
  template <typename T> T *take(uint64_t count) {
    uint64_t at = off;
    off += (count * sizeof(T) + 255) & ~255ull;
    return base ? reinterpret_cast<T *>(base + at) : nullptr;
  }
};

// size the layout, grow the scratch buffer to it, then lay it out for real
template <typename Layout>
int carve_scratch(m3x_ctx *ctx, uint8_t **buf, uint64_t *cur, Layout layout) {
  ScratchCarver sizing{nullptr};
  layout(sizing);
  int rc = ensure_scratch(ctx, buf, cur, sizing.off);
  if (rc != 0) return rc;
  ScratchCarver real{*buf};
  layout(real);
  return 0;
}

// The temporary device buffers of one host-buffer call. The first failed
// allocation or copy is remembered: ok() turns false and later uploads
// return null, so an infrastructure failure surfaces as M3X_ERR_HIP and
// never as a verdict computed over stale device memory. The destructor
// frees everything, on every return path; a caller whose side streams may
// still read a buffer synchronises them before it returns.
class DevTemps {
 public:
  explicit DevTemps(hipStream_t st) : st_(st) {}
  DevTemps(const DevTemps &) = delete;
  DevTemps &operator=(const DevTemps &) = delete;
  ~DevTemps() {
    for (int i = 0; i < n_; i++) (void)hipFree(p_[i]);
  }
  bool ok() const { return ok_; }
  template <typename T = uint8_t> T *alloc(uint64_t bytes) {
    void *d = nullptr;
    if (!ok_ || n_ == kCap || hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) {
      ok_ = false;
      return nullptr;
    }
    p_[n_++] = d;
    return static_cast<T *>(d);
  }
  // device copy of a host buffer; the data is in place on return
  template <typename T> T *upload(const T *host, uint64_t bytes) {
    T *d = alloc<T>(bytes);
    if (d && bytes && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      ok_ = false;
      return nullptr;
    }
    return d;
  }
  // queue a copy back to the host on the call's stream; sync() completes it
  void download(void *dst, const void *src_dev, uint64_t bytes) {
    if (ok_ && hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, st_) != hipSuccess)
      ok_ = false;
  }
  // wait for the stream (always: buffers are about to be freed)
  bool sync() {
    if (hipStreamSynchronize(st_) != hipSuccess) ok_ = false;
    return ok_;
  }
  // hand a buffer over to the caller: the destructor leaves it alone
  template <typename T> T *release(T *d) {
    for (int i = 0; i < n_; i++)
      if (p_[i] == d) p_[i] = p_[--n_];
    return d;
  }

 private:
  static constexpr int kCap = 8;
  hipStream_t st_;
  void *p_[kCap] = {};
  int n_ = 0;
  bool ok_ = true;
};
} // namespace m3x
