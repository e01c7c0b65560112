// The flat search's shortlist bound for inner products ("The flat shortlist bound for
// inner products").  Plain C++ that compiles for the host and the device, so a CPU test can hammer
// the very functions the merge kernels call (tests/test_flat_ip_bound.py, through
// alaya_flat_ip_slack).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALAYA_HD __host__ __device__
#else
#define ALAYA_HD
#endif

namespace alaya_amd {

// contraction codes (alaya_index_flat_last_contraction)
constexpr int kFlatF32 = 0, kFlatSplit = 1, kFlatF16 = 2;

// |s + t| beyond this: the single pass's scale-back 2^-(s + t) leaves f32's range, no bound
constexpr int kFlatF16MaxExp = 100;

// slack(q) with  |d_ref(q, b) + C~(q, b)| <= slack(q)  for every row b with |b| <= b_max, where
// d_ref is the reference's f32 inner-product distance (ip_sqr_avx2) and C~ the scan's contraction
// (0 = f32 MFMA, 1 = bf16 hi/lo split, 2 = single-pass f16 with scale exponents q_exp, base_exp)
// accumulated over k_acc columns.  qn = |q|^2 as an f32 sum.  +inf (or NaN): no bound.
//
//   slack = (A + R) u |q| b_max + (contraction term) + 1e-30, times (1 + 2 k_acc u), with u = 2^-24:
//   A   accumulation of C~: one rounding of at most one ulp (2 u, whatever the matrix unit's
//       rounding mode) per accumulated term, 2 k_acc units, x 1.01 for the second-order terms of
//       (1 + 2u)^k_acc (2 k_acc u <= 2^-7); split: 3 k_acc terms of total magnitude <= 1.008 |q||b|,
//       x 3.1; f16: operands up to (1 + 2^-11) of their f32 values, x 1.01 (k_acc <= 224);
//   R   the reference's sum: at most dim/32 + 3 + 5 + 7 roundings reach a term (32-blocks, 8-blocks,
//       the combine tree, the scalar tail; the products are fused), k_acc/32 + 16 units with one
//       spare for the second order;
//   split: the dropped ql.bl and the two residuals, 3.05 x 2^-16 |q||b|;
//   f16: (2^-10 + 2^-22) |q||b| + (1 + 2^-11) sqrt(K) (a_b |q| + a_q |b|) + K a_q a_b with a_b =
//       2^(-14 - base_exp), a_q = 2^(-14 - q_exp), x 1.0001 for this expression's own roundings;
//   1e-30 covers results rounded in the subnormal range (each within 2^-150) and bf16 lo parts
//       flushed as denormals;
//   (1 + 2 k_acc u) covers the roundings of qn (k_acc/64 + 7 of them, halved by the square root), of
//       b_max's sum (its 1.0001 is applied where it is computed) and of the <= 16 operations here.
ALAYA_HD inline float flat_ip_slack(int contraction, uint32_t k_acc, float qn, int q_exp, float b_max, int base_exp) {
  const float kInf = __builtin_inff();
  if (!(qn >= 0.f) || !(qn < 3.0e38f) || !(b_max >= 0.f) || !(b_max < 3.0e38f)) return kInf;
  if (k_acc == 0 || k_acc > 65536u) return kInf;
  const float u = 5.9604644775390625e-8f;
  const float K = static_cast<float>(k_acc);
  const float qnorm = sqrtf(qn);
  const float qb = qnorm * b_max;
  const float acc = 2.0f * K * (contraction == kFlatSplit ? 3.1f : 1.01f);
  const float ref = static_cast<float>(k_acc / 32u + 16u);
  float s = (acc + ref) * u * qb;
  if (contraction == kFlatF16) {
    if (q_exp + base_exp > kFlatF16MaxExp || q_exp + base_exp < -kFlatF16MaxExp) return kInf;
    const float ec = (9.7680283e-4f + 2.4e-7f) * qb +
                     1.0005f * sqrtf(K) * (ldexpf(qnorm, -14 - base_exp) + ldexpf(b_max, -14 - q_exp)) +
                     ldexpf(K, -28 - base_exp - q_exp);
    s += 1.0001f * ec;
  } else if (contraction == kFlatSplit) {
    s += 3.05f * 1.52587890625e-5f * qb;
  }
  s += 1e-30f;
  return s * (1.0f + 2.0f * K * u);
}

// Whether the shortlist provably holds the exact top-k: kth_d = the k-th returned reference
// distance (FLT_MAX: fewer than k rows), cutoff = a value no row outside the shortlist ranks
// below, in the scan's units -2 C~.  Every outside row then has
//   d_ref >= -C~ - slack >= cutoff / 2 - slack,
// and the query is proven when kth_d is strictly below that.  cutoff / 2 is exact (or within 2^-150,
// inside slack's 1e-30); the subtraction is rounded to nearest, so the float below its result is <=
// the exact difference.  Non-finite values compare false.  cutoff == FLT_MAX: nothing is outside.
ALAYA_HD inline bool flat_ip_proven(float kth_d, float cutoff, float slack) {
  if (cutoff == FLT_MAX) return true;
  if (!(cutoff > -FLT_MAX)) return false;  // an aborted block's unprovable shortlist
  const float rhs = 0.5f * cutoff - slack;
  return kth_d < nextafterf(rhs, -__builtin_inff());
}

}  // namespace alaya_amd
