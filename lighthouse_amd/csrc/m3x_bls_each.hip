// The pairing kernel of the per-set BLS pipeline (m3x_bls_verify_each; the
// rest of that pipeline and its host side are in m3x_bls.hip).
//
// It lives in a translation unit of its own on purpose. The cooperative
// helpers it shares with the batch tail (miller_w, f12_mul_w, final_exp_w)
// are plain `inline` functions: a second caller inside m3x_bls.hip changes
// how the compiler inlines them into k_bls_finish (measured: 272 + 24
// registers and 16 B of scratch became 280 + 32 and 176 B). Here the kernel
// gets the same treatment as k_kzg_finish, which holds the same buffers,
// and the batch kernels compile exactly as before.
#include "bls_device.hh"
#include "m3x_ctx.hh"

using namespace m3xb;

namespace {

// SignatureSet::verify()'s pairing check (generic_signature_set.rs:111-120
// -> fast_aggregate_verify, blst.rs:250-261), ONE WAVE PER SET (the
// k_bls_miller_small / k_kzg_finish shape), n blocks of 64:
//   final_exp(miller(apk_i, H(m_i)) * miller(-g1, sigma_i)) == 1
// Two cooperative Miller loops over one miller_ws, their product, the final
// exponentiation; lane 0 writes the verdict. A set marked by an earlier
// stage writes 0 before any pairing work (wave-uniform branch). The full
// register file and ~46 KiB of LDS per wave: one wave per SIMD, at most
// three blocks per CU.
__global__ __launch_bounds__(64) void k_bls_verify_each(
    uint64_t n, const g1j *__restrict__ apk, const g2j *__restrict__ h2c,
    const g2j *__restrict__ sig_aff, const int32_t *__restrict__ status,
    int32_t *__restrict__ verdicts) {
  __shared__ fp12m sh[7];
  __shared__ f12w_ws ws;
  __shared__ miller_ws mws;
  uint64_t i = blockIdx.x;
  int lane = threadIdx.x;
  if (i >= n) return;
  if (status[i] != 0) {
    if (lane == 0) verdicts[i] = 0;
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
  miller_w(sh[0], apk[i], h2c[i], ws, mws, lane);
  f12w_sync();
  // sig_aff is Jacobian with z = 1, or z = 0 for the infinity signature,
  // for which miller_w returns one
  miller_w(sh[1], ng1, sig_aff[i], ws, mws, lane);
  f12w_sync();
  f12_mul_w(sh[1], sh[0], sh[1], ws, lane);
  final_exp_w(sh[2], sh[1], &sh[3], ws, lane);
  if (lane == 0) verdicts[i] = f12_is_one(sh[2]) ? 1 : 0;
}

} // namespace

namespace m3x {
void launch_bls_verify_each(hipStream_t st, uint64_t n, const g1j *apk,
                            const g2j *h2c, const g2j *sig_aff,
                            const int32_t *status, int32_t *verdicts) {
  hipLaunchKernelGGL(k_bls_verify_each, dim3((uint32_t)n), dim3(64), 0, st, n,
                     apk, h2c, sig_aff, status, verdicts);
}
} // namespace m3x
