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

// The shape parameter of a kind that has one -- RQ's alpha, which follows the d lengthscales in every `lengthscale`
// argument -- read once per thread; empty for the other kinds.  The trend-plus-seasonal kind's one scalar shape value, the
// seasonal outputscale s_s behind its 4 d per-dimension values, travels in `alpha`.
struct PairShape {
  double alpha, inv_2alpha;
};
template <int KIND>
__device__ __forceinline__ PairShape load_pair_shape(const double *__restrict__ lengthscale, int d) {
  if (KIND == PLS_KERNEL_TREND_SEASONAL) return PairShape{lengthscale[4 * d], 0.0};
  if (KIND != PLS_KERNEL_RQ) return PairShape{0.0, 0.0};
  const double alpha = lengthscale[d];
  return PairShape{alpha, 0.5 / alpha};
}

// Rational quadratic (gpytorch's RQKernel times the outputscale): u = r^2 / (2 alpha), kappa = (1 + u)^-alpha =
// exp(-alpha log1p(u)).  log1p: w = fl(1 + u) and e, the exact rounding error of that sum (TwoSum), go to the two-piece
// logarithm of fmath.h -- about 1 ulp down to u -> 0, and log1p(0) = 0, so that kappa = 1 exactly at distance 0.  Dead where
// the exponent underflows or 1 + u overflows (r = inf included): only a large alpha kills a pair, at alpha = ln 2 a point
// 1e4 lengthscales away still has kappa = 3e-6.  q: the pieces of the logarithm, L: log1p(u), for rq_factors.
__device__ __forceinline__ bool rq_kappa(double s2, const PairShape &sh, double &kap, double &u, double &w, LogPieces &q,
                                         double &L) {
  u = s2 * sh.inv_2alpha;
  w = 1.0 + u;
  const double bb = w - 1.0;
  const double e = (1.0 - (w - bb)) + (u - bb);
  q = fast_log_unit_reduce<true>(w, e);
  L = fast_log_unit_combine(q);
  const double x = -sh.alpha * L;
  kap = exp_nonpos_unguarded(x);
  return !(x < -745.2) && w != __builtin_huge_val();
}
// g: dK_ij / d log l_k = outputscale * g * e_k^2 with g = kappa / (1 + u);  ga: dK_ij / d log alpha = outputscale * ga with
// ga = alpha kappa h, h = u / (1 + u) - log1p(u).  h is -u^2 / 2 for small u, where its two terms cancel; there (w < sqrt 2:
// the logarithm's k = 0 and f = u) it is put together from the logarithm's own pieces, log1p(u) = f - hfsq + s (hfsq + R) and
// u / (1 + u) = f - f^2 / (1 + f), so h = hfsq - f^2 / (1 + f) - s (hfsq + R): three terms of size f^2 that cancel to a
// quarter of their sum at the worst, and exactly 0 at distance 0.  From sqrt 2 on the plain difference loses at most 4 bits.
__device__ __forceinline__ void rq_factors(const PairShape &sh, double kap, double u, double w, const LogPieces &q, double L,
                                           double &g, double &ga) {
#pragma clang fp contract(off)
  const double rw = fast_div_normal(1.0, w);
  g = kap * rw;
  const double h = (q.dk == 0.0) ? (q.hfsq - (q.f * q.f) * rw) - q.s * (q.hfsq + q.R) : u * rw - L;
  ga = sh.alpha * kap * h;
}

// sin(pi r) and cos(pi r) for |r| <= 1/2 (gfx950 has no fp64 sine instruction, and the library's sincospi spends most of its
// instructions on an argument reduction that the periodic pair has already done).  u = |r| for |r| <= 1/4, else 1/2 - |r|
// (exact), which swaps the two; on u <= 1/4 the Taylor polynomials of sin(pi u) / u - pi (degree 8 in u^2: truncation 1e-19
// relative) and of cos(pi u) - 1 (degree 8: 3e-18).  pi enters as its two-piece value in ONE fma, u pi_hi + u (pi_lo + ...),
// so the sine is within 0.8 ulp (measured on the CPU against 64-bit-mantissa arithmetic; the cosine's 1 + z q about 1 ulp).
// sin(pi 0) = 0 exactly (with the sign of r), cos(pi / 2) = 0 exactly; a NaN stays NaN.
__device__ __forceinline__ void sincospi_half(double r, double &s, double &c) {
#pragma clang fp contract(off)
  const double a = fabs(r);
  const bool big = a > 0.25;
  const double u = big ? 0.5 - a : a;
  const double z = u * u;
  double p = 7.9520540014755126e-07;  // (-1)^k pi^(2k+1) / (2k+1)!, k = 8 ... 1
  p = fma_k(p, z, -2.1915353447830217e-05);
  p = fma_k(p, z, 4.6630280576761255e-04);
  p = fma_k(p, z, -7.3704309457143504e-03);
  p = fma_k(p, z, 8.2145886611128233e-02);
  p = fma_k(p, z, -5.9926452932079211e-01);
  p = fma_k(p, z, 2.5501640398773455e+00);
  p = fma_k(p, z, -5.1677127800499703e+00);
  const double su = fma(u, 3.1415926535897931, u * fma(p, z, 1.2246467991473532e-16));
  double q = 4.3030695870329473e-06;  // (-1)^k pi^(2k) / (2k)!, k = 8 ... 1
  q = fma_k(q, z, -1.0463810492484570e-04);
  q = fma_k(q, z, 1.9295743094039231e-03);
  q = fma_k(q, z, -2.5806891390014061e-02);
  q = fma_k(q, z, 2.3533063035889321e-01);
  q = fma_k(q, z, -1.3352627688545895e+00);
  q = fma_k(q, z, 4.0587121264167685e+00);
  q = fma_k(q, z, -4.9348022005446790e+00);
  const double cu = fma(q, z, 1.0);
  s = copysign(big ? cu : su, r);
  c = big ? su : cu;
}

// Periodic (gpytorch's PeriodicKernel times the outputscale, as recalled): kappa = exp(-2 sum_k sin^2(pi e_k) / lambda_k),
// e_k = (a_k - b_k) / p_k.  One coordinate from its UNSCALED difference delta, inv_p = 1 / p_k and two_inv_l = 2 / lambda_k:
// difference first, then e = delta inv_p, r = e - rint(e) (|r| <= 1/2, exact), sin and cos of pi r from sincospi_half.
// Returns the coordinate's share of the NEGATED exponent, (2 / lambda_k) sin^2(pi e_k) -- which is also its factor of
// dK / d log lambda_k = s kappa (2 / lambda_k) sin^2(pi e_k) -- and, GRAD only, per = (2 / lambda_k) pi e_k sin(2 pi e_k), its
// factor of dK / d log p_k, with sin(2 pi e) = 2 sin cos of the same evaluation and e itself, unreduced, in front.  Every
// quantity is even in delta, so a pair and its transpose agree bit for bit; a padding coordinate (delta = 0, both scales
// 0) gives 0; a non-finite delta gives NaN (inf - rint(inf)): the kernel has no limit at infinity.
template <bool GRAD>
__device__ __forceinline__ double periodic_coord(double delta, double inv_p, double two_inv_l, double &per) {
#pragma clang fp contract(off)
  const double e = delta * inv_p;
  const double r = e - rint(e);
  double s, c;
  sincospi_half(r, s, c);
  if (GRAD) per = two_inv_l * ((3.1415926535897931 * e) * (2.0 * (s * c)));
  return two_inv_l * (s * s);
}
// kappa from the negated exponent q = sum_k (2 / lambda_k) sin^2(pi e_k) >= 0 (added in ascending k); false: a dead pair
__device__ __forceinline__ bool periodic_kappa(double q, double &kap) {
  const double x = -q;
  kap = exp_nonpos_unguarded(x);
  return !(x < -745.2);
}

// Locally periodic (gpytorch's RBFKernel * PeriodicKernel times the outputscale, as recalled): kappa = exp(-(1/2 sum_k
// ((a_k - b_k) / l_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k)): both factors share the one exponential.  One coordinate from
// its UNSCALED difference delta, inv_l = 1 / l_k and periodic_coord's two scales: z = delta inv_l, the periodic share
// from periodic_coord, and the two shares of the coordinate added in ONE explicit fma, (z / 2) z + share (z / 2 is exact).
// Returns the coordinate's share of the NEGATED exponent; GRAD only: env = z^2, the factor of dK / d log l_k, lam = the
// periodic share, the factor of dK / d log lambda_k, per as periodic_coord's.  Even in delta like periodic_coord; a padding
// coordinate (delta = 0, all scales 0) gives 0; a non-finite delta gives NaN (inf + NaN).
template <bool GRAD>
__device__ __forceinline__ double locally_periodic_coord(double delta, double inv_l, double inv_p, double two_inv_lam,
                                                         double &env, double &lam, double &per) {
#pragma clang fp contract(off)
  const double z = delta * inv_l;
  const double share = periodic_coord<GRAD>(delta, inv_p, two_inv_lam, per);
  if (GRAD) {
    env = z * z;
    lam = share;
  }
  return fma(0.5 * z, z, share);
}

// Trend plus seasonal (gpytorch's ScaleKernel(RBFKernel) + ScaleKernel(RBFKernel * PeriodicKernel), as recalled): k = s_t kappa_t +
// s_s kappa_s with kappa_t = exp(-1/2 sum_k ((a_k - b_k) / l_k)^2) and kappa_s the locally periodic kappa of (m, lambda, p).
// One coordinate from its UNSCALED difference delta: the seasonal share of the NEGATED seasonal exponent is
// locally_periodic_coord's of the same operands (returned; env, lam, per as there), so the seasonal term has the locally
// periodic kind's bits; the trend's distance sum takes z = delta inv_t in one explicit fma, s2 = z z + s2 (GRAD only: tr = z^2,
// the factor of dK / d log l_k).  Even in delta; a padding coordinate (delta = 0, all scales 0) leaves s2 alone and gives 0.
template <bool GRAD>
__device__ __forceinline__ double trend_seasonal_coord(double delta, double inv_t, double inv_m, double inv_p, double two_inv_lam,
                                                       double &s2, double &tr, double &env, double &lam, double &per) {
#pragma clang fp contract(off)
  const double z = delta * inv_t;
  s2 = fma(z, z, s2);
  if (GRAD) tr = z * z;
  return locally_periodic_coord<GRAD>(delta, inv_m, inv_p, two_inv_lam, env, lam, per);
}
// kappa_t from the trend's distance sum s2 >= 0: the RBF exponent -s2 / 2 under the 745.2 rule; false: a dead term
__device__ __forceinline__ bool trend_kappa(double s2, double &kap) {
  const double x = -0.5 * s2;
  kap = exp_nonpos_unguarded(x);
  return !(x < -745.2);
}
// The Gram entry from the trend's distance sum s2 and the seasonal term's negated exponent q: each term takes its own underflow
// decision and a dead one contributes exactly 0; fma(s_t, kappa_t, s_s kappa_s), so that the entry is s_t + s_s rounded once
// at distance 0, the locally periodic entry s_s kappa_s where the trend is dead and s_t kappa_t where the seasonal term is.
__device__ __forceinline__ double trend_seasonal_entry(double s2, double q, double s_t, double s_s) {
  double kt, ks;
  const bool live_t = trend_kappa(s2, kt), live_s = periodic_kappa(q, ks);
  return fma(s_t, live_t ? kt : 0.0, live_s ? s_s * ks : 0.0);
}

// The one front over the three coordinate functions, for every loop over the coordinates of a pair (base_kernel.h, the
// selector): delta is the UNSCALED difference and sc column k of the kind's scale block, one value per parameter block in
// the order of the `lengthscale` argument -- periodic (2 / lambda_k, 1 / p_k), locally periodic (1 / l_k, 2 / lambda_k, 1 / p_k),
// trend plus seasonal (1 / l_k, 1 / m_k, 2 / lambda_k, 1 / p_k).  Returns the coordinate's share of the negated exponent q, adds
// into the trend's distance sum s2 where the kind has one, and (GRAD only) writes f[j], the coordinate's factor of
// dK / d log of block j's parameter.
template <int KIND, bool GRAD, int NS>
__device__ __forceinline__ double pair_coord(double delta, const double (&sc)[NS], double &s2, double (&f)[NS]) {
  if constexpr (KIND == PLS_KERNEL_PERIODIC) {
    static_assert(NS == 2, "periodic: lambda, p");
    const double share = periodic_coord<GRAD>(delta, sc[1], sc[0], f[1]);
    if (GRAD) f[0] = share;
    return share;
  } else if constexpr (KIND == PLS_KERNEL_LOCALLY_PERIODIC) {
    static_assert(NS == 3, "locally periodic: l, lambda, p");
    return locally_periodic_coord<GRAD>(delta, sc[0], sc[2], sc[1], f[0], f[1], f[2]);
  } else {
    static_assert(KIND == PLS_KERNEL_TREND_SEASONAL && NS == 4, "trend plus seasonal: l, m, lambda, p");
    return trend_seasonal_coord<GRAD>(delta, sc[0], sc[1], sc[3], sc[2], s2, f[0], f[1], f[2], f[3]);
  }
}
// The entry of such a kind from the sums of pair_coord over its coordinates: one term, s kappa(q) or 0 for a dead pair; trend
// plus seasonal, its two (sh.alpha holds s_s).
template <int KIND>
__device__ __forceinline__ double coord_entry(double s2, double q, double outputscale, const PairShape &sh) {
  if constexpr (KIND == PLS_KERNEL_TREND_SEASONAL) {
    return trend_seasonal_entry(s2, q, outputscale, sh.alpha);
  } else {
    double kap;
    return periodic_kappa(q, kap) ? outputscale * kap : 0.0;
  }
}

// One pair from its distance sum s2 (RBF: r^2; Matern: t^2 = 2 nu r^2; RQ: r^2, with its shape sh): kap = kappa, the kernel
// without its outputscale; t = sqrt(s2) (Matern only) and ex, the exponential inside kappa, for pair_factors.  Returns
// false for a pair whose exponential underflows: kap is meaningless then and the caller lets the pair contribute exactly
// 0.  A NaN stays NaN.
template <int KIND>
__device__ __forceinline__ bool pair_kappa(double s2, double &kap, double &t, double &ex) {
  static_assert(KIND != PLS_KERNEL_RQ, "the rational-quadratic pair goes through rq_kappa");
  t = (KIND == PLS_KERNEL_RBF_ARD) ? 0.0 : sqrt(s2);
  const double x = (KIND == PLS_KERNEL_RBF_ARD) ? -0.5 * s2 : -t;  // the exponent
  const double p = (KIND == PLS_KERNEL_RBF_ARD) ? 1.0 : matern_poly(KIND, t);
  ex = exp_nonpos_unguarded(x);
  kap = (KIND == PLS_KERNEL_RBF_ARD) ? ex : p * ex;
  return !(x < -745.2);
}
template <int KIND>
__device__ __forceinline__ bool pair_kappa(double s2, const PairShape &sh, double &kap) {
  if constexpr (KIND == PLS_KERNEL_RQ) {
    double u, w, L;
    LogPieces q;
    return rq_kappa(s2, sh, kap, u, w, q, L);
  } else {
    double t, ex;
    return pair_kappa<KIND>(s2, kap, t, ex);
  }
}

// pair_kappa plus g: dK_ij / d log l_k = outputscale * g * e'_k^2 with e'_k the pre-scaled difference, and ga (RQ; 0
// otherwise): dK_ij / d log alpha = outputscale * ga.  A dead pair's e'_k^2 may be inf (0 * inf would be NaN), so the
// caller skips it.
template <int KIND>
__device__ __forceinline__ bool pair_factors(double s2, const PairShape &sh, double &kap, double &g, double &ga) {
  ga = 0.0;
  if constexpr (KIND == PLS_KERNEL_RQ) {
    double u, w, L;
    LogPieces q;
    const bool live = rq_kappa(s2, sh, kap, u, w, q, L);
    rq_factors(sh, kap, u, w, q, L, g, ga);
    return live;
  } else {
    double t, ex;
    const bool live = pair_kappa<KIND>(s2, kap, t, ex);
    if (KIND == PLS_KERNEL_RBF_ARD || KIND == PLS_KERNEL_MATERN32) g = ex;
    else if (KIND == PLS_KERNEL_MATERN12) g = (t > 0.0) ? ex / t : 0.0;  // r = 0: every e_k is 0 and the pair contributes 0
    else g = ex * ((1.0 + t) * (1.0 / 3.0));
    return live;
  }
}

// The Gram entry: outputscale * kappa, 0 for a dead pair.  RBF multiplies the outputscale into the selected 0 and the
// others select after the multiply, so a negative outputscale leaves -0 (RBF) or +0 there, as it always has.
template <int KIND>
__device__ __forceinline__ double gram_entry(double s2, const PairShape &sh, double outputscale) {
  double kap;
  const bool live = pair_kappa<KIND>(s2, sh, kap);
  if (KIND == PLS_KERNEL_RBF_ARD) return outputscale * (live ? kap : 0.0);
  return live ? outputscale * kap : 0.0;
}

}  // namespace plship
