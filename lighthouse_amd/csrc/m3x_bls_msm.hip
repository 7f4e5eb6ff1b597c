// The signature sum of the batch BLS pipeline as a bucket MSM:
//   sig_sum = sum_i r_i * sigma_i,  r_i 64-bit, sigma_i affine G2.
//
// Only the sum is ever used (one pairing e(-g1, sig_sum) per batch), so
// the n independent 64-bit double-and-add chains of k_bls_prep_mults3's
// class A (64 doublings + ~32 mixed adds per set) are not needed. With
// unsigned windows of c = kSigMsmWindowBits bits,
//   sum_i r_i sigma_i = sum_w 2^(c w) * sum_j j * B[w][j],
//   B[w][j] = sum of the sigma_i whose w-th digit is j,
// which costs one mixed add per set and window plus a fixed reduction
// over the (2^c - 1) * ceil(64 / c) buckets.
//
// Five small kernels, all on the caller's stream:
//   hist    -> counts[w][j]            (block-private LDS histograms)
//   scan    -> cursor[w][j]            (one block, exclusive prefix)
//   scatter -> idx, sorted by bucket   (cursor[b] ends at the bucket's end)
//   bucket  -> B[w][j]                 (one wave per bucket)
//   reduce  -> win[w] = 2^(c w) * sum_j j * B[w][j], then their sum
// Digit 0 and infinity signatures (sigdec's placeholder for one that does
// not decode included) are skipped by hist and scatter alike. The order of
// the indices inside a bucket depends on the atomics' arrival order, so the
// Jacobian representative of sig_sum may differ from run to run; the point
// does not.
//
// A translation unit of its own, for the reason m3x_bls_each.hip records.
#include "bls_device.hh"
#include "m3x_ctx.hh"
#include "../../include/m3x_consensus.h"

using namespace m3xb;

namespace {

using m3x::kSigMsmBuckets;
using m3x::kSigMsmDigits;
using m3x::kSigMsmWindowBits;
using m3x::kSigMsmWindows;

constexpr int kSortThreads = 256;
// grid cap of hist and scatter (their blocks stride over the sets): every
// hist block ends with up to kSigMsmBuckets global atomics
constexpr uint32_t kSortMaxBlocks = 128;
constexpr int kScanThreads = 256;
constexpr int kScanPer = kSigMsmBuckets / kScanThreads;
static_assert(kSigMsmBuckets % kScanThreads == 0, "scan chunking");
constexpr int kWinThreads = 128;
// k_bls_msm_hist keeps 4 bytes per bucket in static LDS (64 KiB at most)
static_assert(kSigMsmWindowBits >= 1 && kSigMsmWindowBits <= 11, "window");

__device__ __forceinline__ uint32_t msm_digit(uint64_t r, int w) {
  return (uint32_t)(r >> (kSigMsmWindowBits * w)) & (kSigMsmDigits - 1);
}

__global__ __launch_bounds__(kSortThreads) void k_bls_msm_hist(
    const g2j *__restrict__ sig_aff, const uint64_t *__restrict__ rands,
    uint64_t n, uint32_t *__restrict__ counts) {
  __shared__ uint32_t h[kSigMsmBuckets];
  for (int b = threadIdx.x; b < kSigMsmBuckets; b += kSortThreads) h[b] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kSortThreads) {
    if (g2j_is_inf(sig_aff[i])) continue;
    uint64_t r = rands[i];
#pragma unroll
    for (int w = 0; w < kSigMsmWindows; w++) {
      uint32_t d = msm_digit(r, w);
      if (d) atomicAdd(&h[w * kSigMsmDigits + d], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSigMsmBuckets; b += kSortThreads)
    if (h[b]) atomicAdd(&counts[b], h[b]);
}

// cursor[b] = number of entries in the buckets before b (window-major)
__global__ __launch_bounds__(kScanThreads) void k_bls_msm_scan(
    const uint32_t *__restrict__ counts, uint32_t *__restrict__ cursor) {
  __shared__ uint32_t part[kScanThreads];
  int t = threadIdx.x;
  uint32_t before[kScanPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    before[k] = sum;
    sum += counts[t * kScanPer + k];
  }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    uint32_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t base = part[t] - sum;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) cursor[t * kScanPer + k] = base + before[k];
}

__global__ __launch_bounds__(kSortThreads) void k_bls_msm_scatter(
    const g2j *__restrict__ sig_aff, const uint64_t *__restrict__ rands,
    uint64_t n, uint32_t *__restrict__ cursor, uint32_t *__restrict__ idx) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kSortThreads) {
    if (g2j_is_inf(sig_aff[i])) continue;
    uint64_t r = rands[i];
#pragma unroll
    for (int w = 0; w < kSigMsmWindows; w++) {
      uint32_t d = msm_digit(r, w);
      // hist counted this entry, so pos stays inside the bucket's span
      if (d) idx[atomicAdd(&cursor[w * kSigMsmDigits + d], 1u)] = (uint32_t)i;
    }
  }
}

// one WAVE per bucket (the aggregate_w_body shape): lanes stride over the
// bucket's index list with mixed adds, then an LDS tree. Every bucket slot
// is written on every call; an empty one costs one store. The register
// budget is that of k_bls_prep_mults2 and k_bls_h2c_map_lat, which fill the
// SIMDs two waves each while this runs: a wave here takes the place of one
// of theirs as it retires (at the default budget it took 512 registers and
// had to wait for a SIMD with nothing else on it).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_msm_bucket(
    const g2j *__restrict__ sig_aff, const uint32_t *__restrict__ counts,
    const uint32_t *__restrict__ cursor, const uint32_t *__restrict__ idx,
    g2j *__restrict__ buckets) {
  __shared__ g2j lds[64];
  uint32_t b = blockIdx.x;
  int lane = threadIdx.x;
  uint32_t cnt = counts[b];
  g2j acc;
  g2j_set_inf(acc);
  if (cnt == 0) { // wave-uniform
    if (lane == 0) buckets[b] = acc;
    return;
  }
  uint32_t lo = cursor[b] - cnt; // the scatter left cursor at the end
  for (uint32_t k = lane; k < cnt; k += 64) {
    g2a sig;
    sig_aff_load(sig, sig_aff[idx[lo + k]]);
    g2j_add_aff(acc, acc, sig);
  }
  lds[lane] = acc;
  block_tree_reduce<g2j, 64>(lds, lane, g2j_add_op{});
  if (lane == 0) buckets[b] = lds[0];
}

// one block per window: thread t sums [j]B[w][j] over its digits j (a
// c-bit double-and-add each, no running sum along the digits), an LDS tree
// gives the window sum, thread 0 shifts it into place with c*w doublings
__global__ __launch_bounds__(kWinThreads)
__attribute__((amdgpu_waves_per_eu(2, 2))) void k_bls_msm_window(
    const g2j *__restrict__ buckets, g2j *__restrict__ win) {
  __shared__ g2j lds[kWinThreads];
  int w = blockIdx.x, t = threadIdx.x;
  g2j acc;
  g2j_set_inf(acc);
  for (int j = t; j < kSigMsmDigits; j += kWinThreads) {
    g2j base = buckets[w * kSigMsmDigits + j];
    if (j == 0 || g2j_is_inf(base)) continue;
    g2j m;
    g2j_set_inf(m);
    for (int bit = kSigMsmWindowBits - 1; bit >= 0; bit--) {
      g2j_dbl(m, m);
      if ((j >> bit) & 1) g2j_add(m, m, base);
    }
    g2j_add(acc, acc, m);
  }
  lds[t] = acc;
  block_tree_reduce<g2j, kWinThreads>(lds, t, g2j_add_op{});
  if (t == 0) {
    g2j s = lds[0];
    for (int k = 0; k < kSigMsmWindowBits * w; k++) g2j_dbl(s, s);
    win[w] = s;
  }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_bls_msm_sum(
    const g2j *__restrict__ win, g2j *__restrict__ sig_sum) {
  if (threadIdx.x != 0) return;
  g2j s = win[0];
  for (int w = 1; w < kSigMsmWindows; w++) g2j_add(s, s, win[w]);
  sig_sum[0] = s;
}

} // namespace

namespace m3x {
int launch_bls_sig_msm(hipStream_t st, uint64_t n, const g2j *sig_aff,
                       const uint64_t *rands, const SigMsmWork &m,
                       g2j *sig_sum) {
  if (n == 0 || n > kSigMsmMaxSets) return M3X_ERR_ARG;
  M3X_HIP_CHECK(hipMemsetAsync(m.counts, 0, 4 * kSigMsmBuckets, st));
  uint64_t want = (n + kSortThreads - 1) / kSortThreads;
  uint32_t sblocks = want < kSortMaxBlocks ? (uint32_t)want : kSortMaxBlocks;
  hipLaunchKernelGGL(k_bls_msm_hist, dim3(sblocks), dim3(kSortThreads), 0, st,
                     sig_aff, rands, n, m.counts);
  hipLaunchKernelGGL(k_bls_msm_scan, dim3(1), dim3(kScanThreads), 0, st,
                     m.counts, m.cursor);
  hipLaunchKernelGGL(k_bls_msm_scatter, dim3(sblocks), dim3(kSortThreads), 0,
                     st, sig_aff, rands, n, m.cursor, m.idx);
  hipLaunchKernelGGL(k_bls_msm_bucket, dim3(kSigMsmBuckets), dim3(64), 0, st,
                     sig_aff, m.counts, m.cursor, m.idx, m.buckets);
  hipLaunchKernelGGL(k_bls_msm_window, dim3(kSigMsmWindows),
                     dim3(kWinThreads), 0, st, m.buckets, m.win);
  hipLaunchKernelGGL(k_bls_msm_sum, dim3(1), dim3(64), 0, st, m.win, sig_sum);
  return M3X_OK;
}
} // namespace m3x
