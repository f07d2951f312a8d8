// Per-entry math of the stationary base kernels, shared by the Gram build (plship.hip) and the marginal-likelihood
// gradient reduction (gp_mll.hip).
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
// The Gram kernel folds sqrt(2 nu) into its inverse lengthscales, so that its distance sum is t^2 itself.
constexpr double SQRT3 = 1.7320508075688772935, SQRT5 = 2.2360679774997896964;
__host__ __device__ constexpr double matern_t_scale(int kind) {
  return kind == PLS_KERNEL_MATERN32 ? SQRT3 : kind == PLS_KERNEL_MATERN52 ? SQRT5 : 1.0;
}
__device__ __forceinline__ double matern_poly(int kind, double t) {
  return (kind == PLS_KERNEL_MATERN12) ? 1.0 : (kind == PLS_KERNEL_MATERN32) ? 1.0 + t : fma(t, fma(t, 1.0 / 3.0, 1.0), 1.0);
}

}  // namespace plship
