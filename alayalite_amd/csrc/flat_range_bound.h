// The exact range search's two thresholds on the MFMA scan ("Round 24: the range bound").
// Plain C++ that compiles for the host and the device, so a CPU test can hammer the very function the
// scan's prologue calls (tests/test_flat_range_bound.py, through alaya_flat_range_bound).
#pragma once
#include <cmath>
#include <cstdint>

#include "flat_bound.h"

namespace alaya_amd {

// one float down / up; an infinity (an infinite radius) stays where it is
ALAYA_HD inline float flat_range_step(float x, bool up) {
  const float kInf = __builtin_inff();
  return (x == kInf || x == -kInf) ? x : nextafterf(x, up ? kInf : -kInf);
}

struct FlatRangeBound {
  float lo, hi;  // d~ <= lo: d_ref <= radius proven;  d~ > hi: d_ref > radius proven;  else: compute d_ref
};

// (lo, hi) of one query for the scan's approximate distance d~ against the reference's f32 distance d_ref
// (l2_sqr_avx2 / ip_sqr_avx2), for every row b with |b| <= b_max.  radius: the query's f32 radius; qn: |q|^2
// as an f32 sum; k_acc: the contraction's (padded) width; contraction: kFlatSplit is the one the range scan
// runs, kFlatF32 is accepted (its terms are the split's without the dropped products).
//
// L2: d~ = fl(fl(qn + bn) - 2 C~) with bn = |b|^2 as an f32 sum and C~ the contraction.  With D the
// real-number distance |q - b|^2 and S = (|q| + b_max)^2:
//   |d~ - D| <= E = (gam + nrm) S + drop |q| b_max + 1e-30, times (1 + 2 k_acc u), u = 2^-24:
//     gam   shortlist_eps's: 2 k_acc u x 3.1 (split: 3 k_acc terms of total magnitude <= 1.008 |q||b|, one
//           rounding of at most an ulp each, doubled by the factor 2 of -2 C~; 4 |q||b| <= S);
//     nrm   the roundings of qn and bn (k_acc/64 + 7 each, relative to qn + bn <= S) and the two of d~'s own
//           sum (each relative to at most qn + bn + 2 |C~| <= 1.01 S): (k_acc/32 + 24) u;
//     drop  the dropped ql.bl and the two split residuals, twice 3.05 x 2^-16;
//     1e-30 results rounded in the subnormal range and bf16 lo parts flushed as denormals.
//   |d_ref - D| <= g D with g = (k_acc/32 + 18) u: the reference's sum of non-negative terms -- flat_ip_slack's R
//     (k_acc/32 + 16, the roundings that reach a fused product) and 2u for the element difference, which L2
//     rounds before it squares it.
//   in:   (d~ + E)(1 + g) <= r  <=  d~ <= r (1 - g - 4u) - E                  (1 / (1 + g) >= 1 - g)
//   out:  (d~ - E)(1 - g) >  r  <=  d~ >  r (1 + 1.01 g + 4u) + E + 1e-30     (1 / (1 - g) <= 1 + 1.01 g, g < 2^-12)
//   The 4u in the factors cover the two roundings of the product; the last subtraction / addition is rounded
//   to nearest and stepped once with nextafterf.  The 1e-30 on the out side covers d_ref's own underflow.
//   r < 0: no d_ref is below it (d_ref >= 0 or NaN); the factors are dropped, so lo < r and hi >= r.
// IP: d~ = -C~ and |d_ref + C~| <= slack (flat_ip_slack): lo = r - slack, hi = r + slack, stepped likewise.
//
// No bound (non-finite qn or b_max, |q| or b_max >= 1e18, k_acc out of range): lo = -inf, hi = +inf, every row is
// verified.  A NaN threshold (a NaN radius, inf - inf) compares false on both sides: verified as well.
ALAYA_HD inline FlatRangeBound flat_range_bound(bool ip, float radius, float qn, float b_max, uint32_t k_acc,
                                                int contraction) {
  const float kInf = __builtin_inff();
  FlatRangeBound r{-kInf, kInf};
  if (!(qn >= 0.f) || !(qn < 1.0e36f) || !(b_max >= 0.f) || !(b_max < 1.0e18f)) return r;
  if (k_acc == 0 || k_acc > 65536u) return r;
  if (contraction != kFlatSplit && contraction != kFlatF32) return r;
  if (ip) {
    const float slack = flat_ip_slack(contraction, k_acc, qn, 0, b_max, 0);
    if (!(slack < kInf)) return r;
    r.lo = flat_range_step(radius - slack, false);
    r.hi = flat_range_step(radius + slack, true);
    return r;
  }
  const float u = 5.9604644775390625e-8f;
  const float K = static_cast<float>(k_acc);
  const float qnorm = sqrtf(qn);
  const float s = (qnorm + b_max) * (qnorm + b_max);
  const float gam = 2.0f * K * u * (contraction == kFlatSplit ? 3.1f : 1.0f);
  const float nrm = static_cast<float>(k_acc / 32u + 24u) * u;
  float e = (gam + nrm) * s + 1e-30f;
  if (contraction == kFlatSplit) e += 2.0f * 3.05f * 1.52587890625e-5f * qnorm * b_max;
  e *= 1.0f + 2.0f * K * u;
  const float g = static_cast<float>(k_acc / 32u + 18u) * u;
  const bool neg = radius < 0.f;
  const float in = neg ? radius : radius * (1.0f - g - 4.0f * u);
  const float out = neg ? radius : radius * (1.0f + 1.01f * g + 4.0f * u);
  r.lo = flat_range_step(in - e, false);
  r.hi = flat_range_step(out + (e + 1e-30f), true);
  return r;
}

}  // namespace alaya_amd
