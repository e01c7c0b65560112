// The candidate screen's proven lower bound ("Screening on an f16 row copy").
// Plain C++ that compiles for the host and the device, so a CPU test can hammer the very function
// the search kernel calls (tests/test_screen_bound.py).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALAYA_HD __host__ __device__
#else
#define ALAYA_HD
#endif

namespace alaya_amd {

// Slack in units of u = 2^-24 (the f32 unit roundoff) for a sum of `dim` squared differences in any
// order: dim + 2 roundings reach a term (the difference twice, because it is squared, and at most
// dim - 1 additions; a product rounding or an fma folds into one of them, an unfused product adds
// one), and the 13 spare units pay the second-order terms of (1 + u)^(dim + 3) for dim <= 4096 and
// the roundings of the bound's own multiplications.
ALAYA_HD inline float screen_gamma(uint32_t dim) { return static_cast<float>(dim + 16u) * 5.9604644775390625e-8f; }

// Distances below 2^-80 are not screened: there the absolute error of squares that underflow
// (at most 2 dim 2^-126 per sum, flushed or not) is no longer small against the sum.
constexpr float kScreenTiny = 8.271806125530277e-25f;   // 2^-80
constexpr float kScreenHuge = 1.2676506002282294e30f;   // 2^100: sums near overflow are not screened

// A value that is <= the reference's f32 L2 distance of q and x (l2_sqr_avx2, or any other f32
// summation order of the dim squared differences), given
//   d_tilde = an f32 sum, in any order, of (q_j - y_j)^2 over the row's stored copy y, and
//   e_row  >= ||x - y||_2 (exact real norm; +inf = "no bound for this row").
// Returns 0 -- which is <= every L2 distance and screens nothing out -- whenever it has no bound:
// NaN or huge d_tilde, NaN or infinite e_row, tiny results.  A positive return value therefore also
// says that the row is finite and within the copy's range.
ALAYA_HD inline float screen_lower_bound(float d_tilde, float e_row, uint32_t dim) {
  if (!(d_tilde >= kScreenTiny) || !(d_tilde <= kScreenHuge)) return 0.f;
  if (!(e_row >= 0.f) || !(e_row <= kScreenHuge)) return 0.f;
  const float keep = 1.0f - screen_gamma(dim);              // exact: a multiple of 2^-24 in [1/2, 1)
  const float y = d_tilde * keep;                           // <= D~, the exact sum over the copy
  const float s = sqrtf(y) * (1.0f - 9.5367431640625e-7f);  // (1 - 2^-20) <= sqrt(D~), sqrt within 8 u
  const float t = s - e_row;                                // <= ||q - x|| (1 + u)   (triangle inequality)
  if (!(t > 0.f)) return 0.f;
  const float r = (t * t) * keep;                           // <= D (1 - (dim + 11) u) <= reference sum
  return r >= kScreenTiny ? r : 0.f;
}

}  // namespace alaya_amd
