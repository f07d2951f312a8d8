// lgamma, digamma and X(x) = x digamma(x) for positive arguments, for the per-element code of the Beta cost (cost_device.h), in
// the style of fmath.h: the classical reductions, explicit fma Horner kernels, fast_log / fast_div_normal, no floating-point
// contraction, and none of a library routine's ladders for arguments these callers never pass (x <= 0).
//
//   lgamma   x < 3/4: lgamma(1 + x) - log x;  [3/4, 3): three polynomial pieces of lgamma(1 + u), two of them factored
//            through the zeros at 1 and 2 (u A(u), (u - 1) C(u - 1)), so the result keeps its relative accuracy there;
//            [3, 8): lgamma(x) = lgamma(y) + log((y)(y + 1) ... (x - 1)) with y in [2, 3) -- one logarithm of a product;
//            x >= 8: Stirling's series, eight terms in 1 / x^2 (the ninth is 8e-17 at x = 8).
//   digamma  [1, 2]: (x - x0) P(x - 1) / Q(x - 1), x0 = 1.4616... the zero held in two pieces, P / Q a [6/6] interpolant with
//            positive coefficients (2^-56); (2, 10): psi(x) = psi(y) + sum 1 / (y + k), y in [1, 2), the sum folded into ONE
//            rational num / den by the recurrence (one division); x >= 10: log x - 1 / (2 x) - eight terms in 1 / x^2.
//   X        x psi(x) for x >= 1, and -1 + x psi(1 + x) below: X(0) = -1 exactly, no pole.
// The polynomial coefficients are interpolants at Chebyshev nodes of the stated functions, computed at 60 digits (their
// truncation errors are below 2^-55; tests/test_gpu_beta_cost_elements.py pins every function per element against mpmath).
// The loops take at most 5 (lgamma) and 8 (digamma) rounds and none for NaN, infinities or arguments outside the domain.
// lgamma_pos, digamma_pos and xdigamma_pos are CALLED (__noinline__), their pieces inlined into them: inlined into a step or
// GEMM kernel, the coefficients (about a hundred doubles) stay in registers beside the tile's accumulators and the kernel
// spills by the hundred; as leaf functions they need no stack.
#pragma once
#include <hip/hip_runtime.h>

#include "fmath.h"

namespace plship {

template <int N>
__device__ __forceinline__ double horner(const double (&c)[N], double t) {
  double p = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; --k) p = fma(p, t, c[k]);
  return p;
}

// lgamma(1 + u) for -1/4 <= u < 2
__device__ __forceinline__ double lgamma_1p_unit(double u) {
#pragma clang fp contract(off)
  // lgamma(1 + t) / t on [-1/4, 1/4]
  static constexpr double A[19] = {
      -0.5772156649015329,  0.8224670334241133,   -0.4006856343865315, 0.27058080842771787,  -0.20738555102861042,
      0.16955717701613895,  -0.14404989678670604, 0.12550966713649744, -0.11133426359238932, 0.10009962210510019,
      -0.09095417407951806, 0.08334719848486703,  -0.07692618365330123, 0.07159408341567752, -0.06682232999260808,
      0.06020201298139458,  -0.05663245272474891, 0.07302784334409541, -0.06928380249485716};
  // lgamma(3/2 + t) on [-1/4, 1/4]
  static constexpr double B[17] = {
      -0.12078223763524522,  0.03648997397857653,   0.46740110027233966,   -0.1381327740390564,   0.058712126416770156,
      -0.028952081888204487, 0.01543548416961521,   -0.008622603998319755, 0.004965728853037259,  -0.0029209667836465245,
      0.0017450332606850476, -0.001055026249883388, 0.0006437726262611913, -0.000393885373198391, 0.00024368309474267566,
      -0.00016921254148073332, 0.00010582129400058809};
  // lgamma(2 + t) / t on [-1/4, 1]
  static constexpr double C[19] = {
      0.42278433509846713,   0.32246703342411326,    -0.0673523010531985,   0.020580808427772778,  -0.007385551028599507,
      0.002890510331403923,  -0.0011927539167562245, 0.0005096695159815606, -0.00022315461709994272, 9.945729617804146e-05,
      -4.492756357262131e-05, 2.0513068306908562e-05, -9.444677581609408e-06, 4.3515711994268455e-06, -1.9476792144550864e-06,
      7.886045745500326e-07, -2.568289470127565e-07, 5.671651466346744e-08,  -6.12959707211065e-09};
  if (u < 0.25) return u * horner(A, u);
  if (u < 0.75) return horner(B, u - 0.5);
  const double t = u - 1.0;
  return t * horner(C, t);
}

// lgamma(x) for x > 0, or, PLUS1, lgamma(1 + x) for x >= 0 without the rounding of 1 + x where that matters (x < 2).
// +inf at +inf; x = 0 gives +inf (PLUS1: 0).
__device__ __noinline__ inline double lgamma_pos(double x, bool plus1 = false) {
#pragma clang fp contract(off)
  const double xx = plus1 ? 1.0 + x : x;
  if (xx >= 8.0) {
    const double l = fast_log_unit(xx), r = fast_div_normal(1.0, xx), w = r * r;
    double s = -3617.0 / 122400.0;
    s = fma(s, w, 1.0 / 156.0);
    s = fma(s, w, -691.0 / 360360.0);
    s = fma(s, w, 1.0 / 1188.0);
    s = fma(s, w, -1.0 / 1680.0);
    s = fma(s, w, 1.0 / 1260.0);
    s = fma(s, w, -1.0 / 360.0);
    s = fma(s, w, 1.0 / 12.0);
    const double v = fma(xx - 0.5, l - 1.0, fma(s, r, 0.91893853320467274178 - 0.5));  // (x - 1/2)(log x - 1) - 1/2 = ... - x
    return (xx < __builtin_huge_val()) ? v : xx;
  }
  double u, add = 0.0;
  if (xx >= 3.0) {
    double y = xx, z = 1.0;
    while (y >= 3.0) {
      y -= 1.0;
      z *= y;
    }
    u = y - 1.0;
    add = fast_log_unit(z);
  } else if (!plus1 && x < 0.75) {
    u = x;
    add = -fast_log(x);
  } else {
    u = plus1 ? x : x - 1.0;
  }
  return lgamma_1p_unit(u) + add;
}

// digamma(1 + t) for 0 <= t <= 1
__device__ __forceinline__ double digamma_1p_unit(double t) {
#pragma clang fp contract(off)
  static constexpr double P[7] = {1.2503801375034054,  1.8675925104074453,   0.9711327526262392,    0.21631407251432455,
                                  0.01996408274151926, 0.0005811135063985677, 1.0894678528383955e-06};
  static constexpr double Q[7] = {1.0,                 2.1771665986671342,   1.6630736963665909,     0.5710455727133128,
                                  0.09111902253303285, 0.006100975692434821, 0.00012043151172286901};
  const double d = (t - 0.46163214496836236) - -1.5522348162858677e-17;  // 1 + t - x0, exact next to the zero
  return d * fast_div_normal(horner(P, t), horner(Q, t));
}

// digamma(x) for x >= 1
__device__ __forceinline__ double digamma_ge1(double x) {
#pragma clang fp contract(off)
  if (x >= 10.0) {
    const double l = fast_log_unit(x), r = fast_div_normal(1.0, x), w = r * r;
    double s = 3617.0 / 8160.0;
    s = fma(s, w, -1.0 / 12.0);
    s = fma(s, w, 691.0 / 32760.0);
    s = fma(s, w, -1.0 / 132.0);
    s = fma(s, w, 1.0 / 240.0);
    s = fma(s, w, -1.0 / 252.0);
    s = fma(s, w, 1.0 / 120.0);
    s = fma(s, w, -1.0 / 12.0);
    const double v = fma(s, w, fma(-0.5, r, l));
    return (x < __builtin_huge_val()) ? v : x;
  }
  double y = x, num = 0.0, den = 1.0;
  while (y >= 2.0) {  // psi(y + 1) = psi(y) + 1 / y; the sum of reciprocals as one fraction
    y -= 1.0;
    num = fma(num, y, den);
    den *= y;
  }
  const double base = digamma_1p_unit(y - 1.0);
  return (x >= 2.0) ? base + fast_div_normal(num, den) : base;
}

// digamma(x) for x > 0 (-inf at 0)
__device__ __noinline__ inline double digamma_pos(double x) {
#pragma clang fp contract(off)
  return (x < 1.0) ? digamma_1p_unit(x) - fast_div(1.0, x) : digamma_ge1(x);
}

// X(x) = x digamma(x) for x >= 0: -1 at 0
__device__ __noinline__ inline double xdigamma_pos(double x) {
#pragma clang fp contract(off)
  return (x < 1.0) ? fma(x, digamma_1p_unit(x), -1.0) : x * digamma_ge1(x);
}

}  // namespace plship
