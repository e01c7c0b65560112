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

// ---- The 8-bit screening copy ("Round 8") -----------------------------------
// One record per row: a 16-byte header {e_row, lo, scale, 0} and then `stride` codes, padded to a
// multiple of 64 bytes, so a candidate's e_row and its codes come from one place.
constexpr uint32_t kScreenU8Header = 16;
ALAYA_HD inline uint32_t screen_u8_record_bytes(uint32_t stride) { return (kScreenU8Header + stride + 63u) & ~63u; }

// The f32 value y_j that code c stands for.  The copy kernel (for e_row), the search kernel (for d~)
// and the host test all call this one function, and fmaf is one rounding whatever the compiler
// contracts elsewhere, so y_j is the same f32 everywhere.
ALAYA_HD inline float screen_u8_value(uint32_t c, float lo, float scale) {
  return fmaf(static_cast<float>(c), scale, lo);
}

// The quantiser: lo = the row's min, scale = (max - min) / 255, c = clamp(rint((x - lo) / scale)); a
// constant row has scale 0 and codes 0.  Its quality decides how many candidates the screen drops,
// never whether a drop is right: e_row is measured against the values the codes stand for.
ALAYA_HD inline float screen_u8_scale(float lo, float hi) { return (hi - lo) / 255.0f; }
ALAYA_HD inline uint32_t screen_u8_code(float x, float lo, float scale) {
  if (!(scale > 0.f)) return 0u;
  const float c = rintf((x - lo) / scale);
  return c >= 255.f ? 255u : (c >= 0.f ? static_cast<uint32_t>(c) : 0u);  // NaN -> 0
}

// e_row from `sum`, an f32 sum in any order of fl(fl(x_j - y_j)^2) over the row's `stride` elements:
// an over-estimate of ||x - y||_2 by the same slacks as the f16 copy's (1 + screen_gamma on the
// sum, 1 + 2^-19 on its root, 2^-50 for the root of the squares that underflow).  `bad` = an element,
// lo or scale is not finite: +inf, the row is never screened out.
ALAYA_HD inline float screen_u8_err(float sum, uint32_t stride, bool bad) {
  const float err = sqrtf(sum * (1.0f + screen_gamma(stride))) * (1.0f + 1.9073486328125e-6f) + 8.8817841970012523e-16f;
  return (bad || !(err <= kScreenHuge)) ? INFINITY : err;
}
ALAYA_HD inline bool screen_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// ---- The integer screen over the 8-bit records ("Round 10") -------------------
// The query is quantised once with the row functions above (qlo, qs, codes a_j, and e_q from
// screen_u8_err), and a record carries its code sums C1 = sum c_j and C2 = sum c_j^2 as two u32 right
// after its codes, in the padding every screened width has.
ALAYA_HD inline uint32_t screen_u8_sums_offset(uint32_t stride) { return kScreenU8Header + stride; }

// A value <= D^ = ||q^ - y^||^2 over the real-valued grids q^_j = qlo + qs a_j, y^_j = lo + s c_j of
// n <= 4096 elements, from the exact integer sums A1 = sum a, A2 = sum a^2, C1 = sum c, C2 = sum c^2,
// AC = sum a c (all below 2^28) and delta = qlo - lo:
//   D^ = n delta^2 + 2 delta (qs A1 - s C1) + qs^2 A2 + s^2 C2 - 2 qs s AC.
// Six terms in f64.  The products of two f32 values, and of an f32 value and an integer below 2^28,
// are exact there, so a term carries at most 4 roundings (n delta delta: delta's own twice, two
// products), the sum 5 more, the magnitude sum, its scaling and the subtraction 7 more: 16 units of
// 2^-53 of sum |terms| = 2^-49 of it, subtracted explicitly, so cancellation between the terms cannot
// hide them.  (1 - 2^-23) pays the rounding to f32.  0 = "no bound": not positive, or not finite.
ALAYA_HD inline float screen_int_distance(uint32_t n, float qlo, float qs, uint32_t a1, uint32_t a2, float lo,
                                          float s, uint32_t c1, uint32_t c2, uint32_t ac) {
  const double delta = static_cast<double>(qlo) - static_cast<double>(lo);
  const double dq = qs, dr = s;
  const double t1 = (static_cast<double>(n) * delta) * delta;
  const double t2 = (2.0 * delta) * (dq * static_cast<double>(a1));
  const double t3 = (2.0 * delta) * (dr * static_cast<double>(c1));
  const double t4 = (dq * dq) * static_cast<double>(a2);
  const double t5 = (dr * dr) * static_cast<double>(c2);
  const double t6 = (2.0 * (dq * dr)) * static_cast<double>(ac);
  const double sum = ((t1 + t4) + t5) + ((t2 - t3) - t6);
  const double mag = ((t1 + t4) + t5) + ((fabs(t2) + fabs(t3)) + t6);
  const double d = (sum - mag * 1.7763568394002505e-15) * (1.0 - 1.1920928955078125e-7);  // 2^-49, 2^-23
  if (!(d > 0.0) || !(d <= static_cast<double>(kScreenHuge))) return 0.f;
  return static_cast<float>(d);
}

// A value >= ||x - y^|| + ||q - q^||, the two triangle steps from the grids to the row and the query.
// e_row and e_q (screen_u8_err) are measured against the f32 values y_j = screen_u8_value(c_j, lo, s),
// one rounding away from the grid: |y_j - y^_j| <= 2^-24 |y^_j| (or 2^-126 where the f32 result is not
// normal) and |y^_j| <= M = max(|lo|, |lo + 255 s|), so ||y - y^|| <= sqrt(n) (2^-24 M + 2^-126)
// <= 2^-18 M + 2^-120 for n <= 4096; the same for the query.  2^-100 pays both floors, (1 + 2^-22)
// the f64 roundings (under ten) and the rounding to f32.  +inf or NaN in = the same out = no bound.
ALAYA_HD inline float screen_int_err(float e_row, float lo, float s, float e_q, float qlo, float qs) {
  const double m_row = fmax(fabs(static_cast<double>(lo)), fabs(static_cast<double>(lo) + 255.0 * static_cast<double>(s)));
  const double m_q = fmax(fabs(static_cast<double>(qlo)), fabs(static_cast<double>(qlo) + 255.0 * static_cast<double>(qs)));
  const double e = ((static_cast<double>(e_row) + static_cast<double>(e_q)) + ((m_row + m_q) * 3.814697265625e-6 +
                                                                            7.888609052210118e-31)) *
                   (1.0 + 2.384185791015625e-7);  // 2^-18, 2^-100, 2^-22
  return static_cast<float>(e);
}

// The integer screen's bound: <= the reference's f32 L2 distance of q and x.  screen_lower_bound needs
// of its first argument only that it is <= D~ (1 + u)^(n + 2) for the D~ its e_row belongs to; here
// D~ = D^ and screen_int_distance is <= D^ itself.
ALAYA_HD inline float screen_int_bound(uint32_t n, float e_q, float qlo, float qs, uint32_t a1, uint32_t a2, float e_row,
                                       float lo, float s, uint32_t c1, uint32_t c2, uint32_t ac) {
  return screen_lower_bound(screen_int_distance(n, qlo, qs, a1, a2, lo, s, c1, c2, ac),
                            screen_int_err(e_row, lo, s, e_q, qlo, qs), n);
}

}  // namespace alaya_amd
