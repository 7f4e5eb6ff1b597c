// A/B lab for the per-lane Miller kernel (not part of the product build):
// the formulas the product used before the reduced-multiply tower
// (schoolbook f6_mul, 18-product line, xi^-1 in the line, separate line and
// g2j_dbl; a private copy below) against the product's current miller_raw,
// on 64k synthetic (timing-valid) point pairs. Prints each kernel's time.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I lighthouse_amd/csrc \
//     tools/millerlab.hip -o tools/millerlab
#include <hip/hip_runtime.h>
#include <cstdio>
#include "bls_device.hh"
using namespace m3xb;

// ---- the earlier formulas, kept here only as the timing baseline ----
namespace before {

__device__ __forceinline__ void f6_mul(fp6 &r, const fp6 &a, const fp6 &b) {
  fp2 acc[5], t;
  for (int i = 0; i < 5; i++) fp2_zero(acc[i]);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      fp2_mul(t, a.c[i], b.c[j]);
      fp2_add(acc[i + j], acc[i + j], t);
    }
  fp2_mul_xi(t, acc[3]);
  fp2_add(r.c[0], acc[0], t);
  fp2_mul_xi(t, acc[4]);
  fp2_add(r.c[1], acc[1], t);
  r.c[2] = acc[2];
}

__device__ inline void f12_sqr_nn(fp12m &r, const fp12m &a) {
  fp6 A, B, m1, t, u, even, odd;
  f12_split(a, A, B);
  before::f6_mul(m1, A, B);
  f6_add(t, A, B);
  f6_mul_v(u, B);
  f6_add(u, A, u);
  before::f6_mul(t, t, u);
  f6_sub(t, t, m1);
  f6_mul_v(u, m1);
  f6_sub(even, t, u);
  f6_add(odd, m1, m1);
  f12_join(r, even, odd);
}

__device__ inline void f12_line_nn(fp12m &r, const fp12m &f, const fp2 &a0,
                                   const fp2 &a3, const fp2 &a5) {
  for (int k = 0; k < 6; k++) {
    fp2 acc, fk, t;
    f12_get(f, k, fk);
    fp2_mul(acc, fk, a0);
    f12_get(f, (k + 3) % 6, fk);
    fp2_mul(t, fk, a3);
    if (k < 3) fp2_mul_xi(t, t);
    fp2_add(acc, acc, t);
    f12_get(f, (k + 1) % 6, fk);
    fp2_mul(t, fk, a5);
    if (k < 5) fp2_mul_xi(t, t);
    fp2_add(acc, acc, t);
    f12_set(r, k, acc);
  }
}

__device__ inline void miller_raw(fp12m &out, fp12m &tmp, const g1j &Pj,
                                  const g2j &Qj) {
  f12_one(out);
  if (fp_is_zero(Pj.z) || fp2_is_zero(Qj.z)) return;
  g2j T = Qj;
  fp2 xi_inv, xi_inv_zp3, zq2, zq3;
  FP_LOAD_C(xi_inv.c0, FP_TWO_INV);
  fp_neg(xi_inv.c1, xi_inv.c0);
  fp2_sqr(zq2, Qj.z);
  fp2_mul(zq3, zq2, Qj.z);
  fp zp2, zp3, xp, yp = Pj.y;
  fp_sqr(zp2, Pj.z);
  fp_mul(zp3, zp2, Pj.z);
  fp_mul(xp, Pj.x, Pj.z);
  fp2_mul_fp(xi_inv_zp3, xi_inv, zp3);
  fp12m *cur = &out, *tm = &tmp;
  for (int i = 62; i >= 0; i--) {
    before::f12_sqr_nn(*tm, *cur);
    {
      fp12m *sw = cur;
      cur = tm;
      tm = sw;
    }
    {
      fp2 X2, Y2, Z2, Z3, a0, a3, a5, t, t2;
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
      before::f12_line_nn(*tm, *cur, a0, a3, a5);
      {
        fp12m *sw = cur;
        cur = tm;
        tm = sw;
      }
      g2j_dbl(T, T);
    }
    if ((BLS_X_ABS >> i) & 1) {
      fp2 Z2, Z3, Hs, Ms, HZq, a0, a3, a5, t, t2;
      fp2_sqr(Z2, T.z);
      fp2_mul(Z3, Z2, T.z);
      fp2_mul(t, T.x, zq2);
      fp2_mul(t2, Qj.x, Z2);
      fp2_sub(Hs, t, t2);
      fp2_mul(t, T.y, zq3);
      fp2_mul(t2, Qj.y, Z3);
      fp2_sub(Ms, t, t2);
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
      before::f12_line_nn(*tm, *cur, a0, a3, a5);
      {
        fp12m *sw = cur;
        cur = tm;
        tm = sw;
      }
      g2j_add(T, T, Qj);
    }
  }
  f12_conj6_ip(*cur);
  if (cur != &out) f12_copy(out, *cur);
}

} // namespace before

__global__ void k_fill(g1j *p, g2j *q, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // arbitrary in-range field values: the Miller instruction stream does
  // not branch on point validity (only on infinity), so timing holds
  uint64_t s = i * 0x9E3779B97F4A7C15ULL + 12345;
  fp v;
#pragma unroll
  for (int k = 0; k < 6; k++) { s ^= s >> 12; s *= 0x2545F4914F6CDD1DULL; v.v[k] = s; }
  v.v[5] %= BLS_P[5];
  p[i].x = v; p[i].y = v; fp_one(p[i].z);
  q[i].x.c0 = v; q[i].x.c1 = v; q[i].y.c0 = v; q[i].y.c1 = v; fp2_one(q[i].z);
}

__global__ __launch_bounds__(64, 1) void k_miller_before(const g1j *p,
                                                         const g2j *q,
                                                         fp12m *f,
                                                         uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12m acc, tmp;
  before::miller_raw(acc, tmp, p[i], q[i]);
  f[i] = acc;
}

__global__ __launch_bounds__(64, 1) void k_miller_now(const g1j *p,
                                                      const g2j *q, fp12m *f,
                                                      uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12m acc;
  miller_raw(acc, p[i], q[i]);
  f[i] = acc;
}

#define LAB_CHECK(e)                                                           \
  do {                                                                         \
    hipError_t _e = (e);                                                       \
    if (_e != hipSuccess) {                                                    \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e));                  \
      return 1;                                                                \
    }                                                                          \
  } while (0)

int main() {
  const uint64_t n = 65536;
  const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  g1j *p; g2j *q; fp12m *f;
  LAB_CHECK(hipMalloc(&p, n * sizeof(g1j)));
  LAB_CHECK(hipMalloc(&q, n * sizeof(g2j)));
  LAB_CHECK(hipMalloc(&f, n * sizeof(fp12m)));
  hipLaunchKernelGGL(k_fill, grid, block, 0, 0, p, q, n);
  LAB_CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  LAB_CHECK(hipEventCreate(&e0));
  LAB_CHECK(hipEventCreate(&e1));
  // alternate the two so clock drift hits both alike; rep 0 is the warm-up
  for (int rep = 0; rep < 4; rep++) {
    float ms;
    LAB_CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_miller_before, grid, block, 0, 0, p, q, f, n);
    LAB_CHECK(hipEventRecord(e1));
    LAB_CHECK(hipEventSynchronize(e1));
    LAB_CHECK(hipEventElapsedTime(&ms, e0, e1));
    printf("miller_before rep %d: %.2f ms\n", rep, ms);
    LAB_CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_miller_now, grid, block, 0, 0, p, q, f, n);
    LAB_CHECK(hipEventRecord(e1));
    LAB_CHECK(hipEventSynchronize(e1));
    LAB_CHECK(hipEventElapsedTime(&ms, e0, e1));
    printf("miller_now    rep %d: %.2f ms\n", rep, ms);
  }
  return 0;
}
