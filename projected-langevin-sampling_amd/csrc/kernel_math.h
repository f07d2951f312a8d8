// Per-pair math of the stationary base kernels: pair_kappa is the one place that turns a distance sum into kappa and decides
// whether the pair underflowed, for the Gram build, the gradient reduction and the fused mean alike (base_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/plship.h"
#include "fmath.h"

namespace plship {

// exp(x) for x <= 0 (the RBF exponent): n = rint(x log2 e), r = x - n ln 2 (two-piece ln 2), degree-13 Taylor polynomial
// in Horner form (|r| <= 0.347: truncation 4e-18 relative), scaled by 2^n with v_ldexp (gradual underflow as libm).
// Within 1 ulp of the correctly rounded value; about half the instructions of the library exp (no special-case
// ladder, constants in scalar registers).  exp_nonpos_unguarded is the same without the underflow select: meaningless
// below x = -745.2, where the caller selects 0 itself.
__device__ __forceinline__ double exp_nonpos_unguarded(double x) {
  const double n = rint(x * 1.4426950408889634074);
  double r = fma(n, -6.93147180369123816490e-01, x);
  r = fma(n, -1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;  // 1/13!
  p = fma_k(p, r, 2.0876756987868098e-09);
  p = fma_k(p, r, 2.5052108385441720e-08);
  p = fma_k(p, r, 2.7557319223985893e-07);
  p = fma_k(p, r, 2.7557319223985888e-06);
  p = fma_k(p, r, 2.4801587301587302e-05);
  p = fma_k(p, r, 1.9841269841269841e-04);
  p = fma_k(p, r, 1.3888888888888889e-03);
  p = fma_k(p, r, 8.3333333333333332e-03);
  p = fma_k(p, r, 4.1666666666666664e-02);
  p = fma_k(p, r, 1.6666666666666666e-01);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}
__device__ __forceinline__ double exp_nonpos(double x) {
  const double v = exp_nonpos_unguarded(x);
  return (x < -745.2) ? 0.0 : v;
}

// Matern-nu (gpytorch's MaternKernel times the outputscale): with r = |(a - b) / lengthscale| and t = sqrt(2 nu) r,
// k = outputscale * p(t) exp(-t), p = 1 (nu = 1/2), 1 + t (3/2), 1 + t (1 + t/3) (5/2) in Horner form.  Where exp(-t)
// underflows (t > 745.2, r = inf included) the entry is selected to 0 -- p(inf) * 0 would be NaN; a NaN t stays NaN.
// The pairwise kernels fold sqrt(2 nu) into their inverse lengthscales, so that their distance sum is t^2 itself.
constexpr double SQRT3 = 1.7320508075688772935, SQRT5 = 2.2360679774997896964;
__host__ __device__ constexpr double matern_t_scale(int kind) {
  return kind == PLS_KERNEL_MATERN32 ? SQRT3 : kind == PLS_KERNEL_MATERN52 ? SQRT5 : 1.0;
}
__device__ __forceinline__ double matern_poly(int kind, double t) {
  return (kind == PLS_KERNEL_MATERN12) ? 1.0 : (kind == PLS_KERNEL_MATERN32) ? 1.0 + t : fma(t, fma(t, 1.0 / 3.0, 1.0), 1.0);
}

// One pair from its distance sum s2 (RBF: r^2; Matern: t^2 = 2 nu r^2): kap = kappa, the kernel without its outputscale;
// t = sqrt(s2) (Matern only) and ex, the exponential inside kappa, for pair_factors.  Returns false for a pair whose
// exponential underflows: kap is meaningless then and the caller lets the pair contribute exactly 0.  A NaN stays NaN.
template <int KIND>
__device__ __forceinline__ bool pair_kappa(double s2, double &kap, double &t, double &ex) {
  t = (KIND == PLS_KERNEL_RBF_ARD) ? 0.0 : sqrt(s2);
  const double x = (KIND == PLS_KERNEL_RBF_ARD) ? -0.5 * s2 : -t;  // the exponent
  const double p = (KIND == PLS_KERNEL_RBF_ARD) ? 1.0 : matern_poly(KIND, t);
  ex = exp_nonpos_unguarded(x);
  kap = (KIND == PLS_KERNEL_RBF_ARD) ? ex : p * ex;
  return !(x < -745.2);
}
template <int KIND>
__device__ __forceinline__ bool pair_kappa(double s2, double &kap) {
  double t, ex;
  return pair_kappa<KIND>(s2, kap, t, ex);
}

// pair_kappa plus g: dK_ij / d log l_k = outputscale * g * e'_k^2 with e'_k the pre-scaled difference.  A dead pair's
// e'_k^2 may be inf (0 * inf would be NaN), so the caller skips it.
template <int KIND>
__device__ __forceinline__ bool pair_factors(double s2, double &kap, double &g) {
  double t, ex;
  const bool live = pair_kappa<KIND>(s2, kap, t, ex);
  if (KIND == PLS_KERNEL_RBF_ARD || KIND == PLS_KERNEL_MATERN32) g = ex;
  else if (KIND == PLS_KERNEL_MATERN12) g = (t > 0.0) ? ex / t : 0.0;  // r = 0: every e_k is 0 and the pair contributes 0
  else g = ex * ((1.0 + t) * (1.0 / 3.0));
  return live;
}

// The Gram entry: outputscale * kappa, 0 for a dead pair.  RBF multiplies the outputscale into the selected 0 and Matern
// selects after the multiply, so a negative outputscale leaves -0 (RBF) or +0 (Matern) there, as it always has.
template <int KIND>
__device__ __forceinline__ double gram_entry(double s2, double outputscale) {
  double kap;
  const bool live = pair_kappa<KIND>(s2, kap);
  if (KIND == PLS_KERNEL_RBF_ARD) return outputscale * (live ? kap : 0.0);
  return live ? outputscale * kap : 0.0;
}

}  // namespace plship
