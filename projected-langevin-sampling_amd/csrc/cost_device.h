// Cost functions, their derivatives and the link functions, evaluated per element on the device.
// Reference: src/projected_langevin_sampling/costs/*.py and link_functions.py (lines cited per branch).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "fmath.h"
#include "special_device.h"

#include "../../include/plship.h"

namespace plship {

struct CostP {
  int cost, link, mode;
  double p0, p1, p2, p3, jitter;
  double ip0;  // 1 / p0 (Gaussian: 1 / sigma2), computed on the host
  double mm_l1, mm_l2, mm_norm, mm_is2;  // multimodal: log p2, log(1 - p2), 0.5 log(2 pi s2), 1 / s2 (host)
                                         // negative binomial: mm_l1 = log r (host), the others unused
                                         // beta: mm_l1 = log phi (host), the others unused
};

__host__ inline CostP make_costp(const pls_cost_desc *d) {
  CostP c;
  c.cost = d->cost;
  c.link = d->link;
  c.mode = d->deriv_mode;
  c.p0 = d->p[0];
  c.p1 = d->p[1];
  c.p2 = d->p[2];
  c.p3 = d->p[3];
  c.jitter = d->jitter;
  c.ip0 = (d->p[0] != 0.0) ? 1.0 / d->p[0] : 0.0;
  c.mm_l1 = c.mm_l2 = c.mm_norm = c.mm_is2 = 0.0;
  if (d->cost == PLS_COST_MULTIMODAL) {
    const double s2 = d->p[0] * d->p[0];
    c.mm_l1 = std::log(d->p[2]);
    c.mm_l2 = std::log(1.0 - d->p[2]);
    c.mm_norm = 0.5 * std::log(2.0 * 3.14159265358979323846 * s2);
    c.mm_is2 = 1.0 / s2;
  }
  if (d->cost == PLS_COST_NEGATIVE_BINOMIAL || d->cost == PLS_COST_BETA) c.mm_l1 = std::log(d->p[0]);
  return c;
}

// THE list of the (cost, link) pairs with kernel instantiations of their own (the pairs the reference's experiments use, and
// negative binomial/exp, beta/sigmoid, ordinal/identity and gamma/exp -- the only links the ordinal and the Gamma cost are
// accepted with):
// f(integral_constant<COST>, integral_constant<LINK>) for one of them, f(-1, -1) -- the instantiation that switches at run
// time -- for every other pair; Beta under another link gets f(PLS_COST_BETA, -1), which switches the link only (the
// run-time-switch instantiation does not carry the Beta code).  Every launcher that dispatches on the pair goes through here.
template <class F>
__host__ inline int for_cost_link(const CostP &cp, F &&f) {
  using std::integral_constant;
  const int c = cp.cost, l = cp.link;
  if (c == PLS_COST_GAUSSIAN && l == PLS_LINK_IDENTITY) return f(integral_constant<int, PLS_COST_GAUSSIAN>{}, integral_constant<int, PLS_LINK_IDENTITY>{});
  if (c == PLS_COST_POISSON && l == PLS_LINK_SQUARE) return f(integral_constant<int, PLS_COST_POISSON>{}, integral_constant<int, PLS_LINK_SQUARE>{});
  if (c == PLS_COST_BERNOULLI && l == PLS_LINK_SIGMOID) return f(integral_constant<int, PLS_COST_BERNOULLI>{}, integral_constant<int, PLS_LINK_SIGMOID>{});
  if (c == PLS_COST_BERNOULLI && l == PLS_LINK_PROBIT) return f(integral_constant<int, PLS_COST_BERNOULLI>{}, integral_constant<int, PLS_LINK_PROBIT>{});
  if (c == PLS_COST_STUDENT_T && l == PLS_LINK_IDENTITY) return f(integral_constant<int, PLS_COST_STUDENT_T>{}, integral_constant<int, PLS_LINK_IDENTITY>{});
  if (c == PLS_COST_MULTIMODAL && l == PLS_LINK_IDENTITY) return f(integral_constant<int, PLS_COST_MULTIMODAL>{}, integral_constant<int, PLS_LINK_IDENTITY>{});
  if (c == PLS_COST_NEGATIVE_BINOMIAL && l == PLS_LINK_EXP) return f(integral_constant<int, PLS_COST_NEGATIVE_BINOMIAL>{}, integral_constant<int, PLS_LINK_EXP>{});
  if (c == PLS_COST_BETA && l == PLS_LINK_SIGMOID) return f(integral_constant<int, PLS_COST_BETA>{}, integral_constant<int, PLS_LINK_SIGMOID>{});
  if (c == PLS_COST_BETA) return f(integral_constant<int, PLS_COST_BETA>{}, integral_constant<int, -1>{});  // (the link at run time)
  if (c == PLS_COST_ORDINAL && l == PLS_LINK_IDENTITY) return f(integral_constant<int, PLS_COST_ORDINAL>{}, integral_constant<int, PLS_LINK_IDENTITY>{});
  if (c == PLS_COST_GAMMA && l == PLS_LINK_EXP) return f(integral_constant<int, PLS_COST_GAMMA>{}, integral_constant<int, PLS_LINK_EXP>{});
  return f(integral_constant<int, -1>{}, integral_constant<int, -1>{});
}

__device__ inline double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// link_functions.py:30-80.  *slope receives d link / d f as torch autograd sees it (0 outside the clip).
// (No floating-point contraction in link_eval / cost_value / cost_deriv: a kernel that evaluates value AND derivative shares
// their common subexpressions, and whether `a * b + c` becomes one fma depends on how many uses the product has -- left to the
// compiler, asking a step for the energy of its input could move the step by an ulp.)
__device__ inline double link_eval(int link, double f, double jit, double *slope) {
#pragma clang fp contract(off)
  switch (link) {
    case PLS_LINK_IDENTITY:  // :54-55
      *slope = 1.0;
      return f;
    case PLS_LINK_SQUARE:  // :79-80
      *slope = 2.0 * f;
      return f * f;
    case PLS_LINK_SIGMOID: {  // :67-70
      const double ex = fast_exp(-f);
      double raw = fast_div(1.0, 1.0 + ex);
      bool inside = (raw >= jit) && (raw <= 1.0 - jit);
      // d/df 1/(1+e^-f) = e^-f / (1+e^-f)^2, the form autograd differentiates (raw*(1-raw) cancels near raw = 1)
      *slope = inside ? ex * raw * raw : 0.0;
      return clipd(raw, jit, 1.0 - jit);
    }
    case PLS_LINK_PROBIT: {  // :39-45
      double raw = 0.5 * (1.0 + erf(f * 0.70710678118654752440));
      bool inside = (raw >= jit) && (raw <= 1.0 - jit);
      *slope = inside ? 0.39894228040143267794 * fast_exp(-0.5 * f * f) : 0.0;
      return clipd(raw, jit, 1.0 - jit);
    }
    case PLS_LINK_EXP: {  // not in the reference: p = exp(f), no clip (+inf above the fp64 range, gradual underflow)
      const double p = fast_exp(f);
      *slope = p;
      return p;
    }
    default:  // (the host entries refuse every other id)
      *slope = __builtin_nan("");
      return __builtin_nan("");
  }
}

// log(1 + x) for x >= 0 (+inf included; NaN for NaN and for x < -1): the sum 1 + x held in two pieces, so the bits of x below
// ulp(1) reach the logarithm (log1p(x) = x for x < 2^-53, and no cancellation against log 1 = 0)
__device__ inline double log1p_pos(double x) {
#pragma clang fp contract(off)
  const double hi = fmax(x, 1.0), lo = fmin(x, 1.0);
  const double s = hi + lo;
  const double e = lo - (s - hi);
  const double v = fast_log_unit_tail(s, e);
  return (x < __builtin_huge_val() && s > 0.0) ? v : (x == -1.0 ? -__builtin_huge_val() : x >= 0.0 ? x : __builtin_nan(""));
}

// The negative binomial under the exponential link, in t = f - log r (mu / r = e^t; mu itself is never formed: it overflows
// from f = 709.8 and underflows from f = -745.2, where value and derivative are finite):
//   cost  = r log1p(e^t) + y log1p(e^-t) = r softplus(t) + y softplus(-t),   softplus(+-t) = max(+-t, 0) + log1p(e^-|t|)
//   cost' = r sigma(t) - y sigma(-t),   sigma(|t|) = 1 / (1 + e^-|t|),   sigma(-|t|) = e^-|t| / (1 + e^-|t|)
// One exponential e = e^-|t| in (0, 1]; 1 + e in two pieces (s, tail) for the logarithm.  The value is r t for large t and
// -y t for large -t (0 * max(-t, 0) = 0 for y = 0 however large -t is); the derivative stays in [-y, r].
struct NbExp {
  double e, s, tail;
  bool pos;
};
__device__ inline NbExp nb_exp_reduce(double t) {
#pragma clang fp contract(off)
  NbExp q;
  q.e = fast_exp(-fabs(t));
  q.s = 1.0 + q.e;
  q.tail = q.e - (q.s - 1.0);
  q.pos = t >= 0.0;
  return q;
}
__device__ inline double nb_exp_value(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  const double t = f - c.mm_l1;
  const NbExp q = nb_exp_reduce(t);
  const double l = fast_log_unit_tail(q.s, q.tail);  // log1p(e^-|t|) in [0, log 2]
  const double up = q.pos ? t + l : l, dn = q.pos ? l : l - t;  // softplus(t), softplus(-t)
  const double a = c.p0 * up, b = y * dn;
  return (y == 0.0) ? a : a + b;  // (y = 0: the second term is exactly 0, also where softplus(-t) is +inf)
}
__device__ inline double nb_exp_deriv(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  const double t = f - c.mm_l1;
  const NbExp q = nb_exp_reduce(t);
  const double big = fast_div_normal(1.0, q.s), small = q.e * big;  // sigma(|t|), sigma(-|t|); 1 <= s <= 2
  const double a = c.p0 * (q.pos ? big : small), b = y * (q.pos ? small : big);
  return a - b;
}

// The Beta cost (mean-precision form, plship.h) under the sigmoid link, evaluated in f without the link's clip.  y holds
// z = logit of the observed proportion.  One exponential e = e^-|f| in (0, 1]: mu_s = e / (1 + e) <= 1/2 <= mu_b = 1 / (1 + e)
// are the smaller and the bigger of (mu, 1 - mu), a_s = phi mu_s, a_b = phi mu_b the two shapes, w = phi mu_s mu_b:
//   cost  = [lgamma(1 + a_s) - log a_s] + lgamma(a_b) - (f >= 0 ? a_b : a_s) z
//           log a_s = log phi - |f| - log1p(e) from its parts: finite where a_s underflows (the cost grows like |f|)
//   cost' = sg (mu_s X(a_b) - mu_b X(a_s)) - w z,   X(x) = x psi(x) = -1 + x psi(1 + x) below 1,  sg = +1 for f >= +-0
//           (mu_s X(a_b) = w psi(a_b)); X(a_s) -> -1 in the tails, so cost' -> sg exactly: the drift is bounded
// The two lgamma and the two X calls run as two rounds of one loop: one copy of the special-function code per function.
// A kernel that asks for value and derivative calls both functions with the same arguments: the reduction (the exponential
// and the division) is the same expression in both and is evaluated once.
// The Beta code is NOT a case of cost_value / cost_deriv: those two, and with them every kernel of every other pair and the
// run-time-switch instantiations, are what they were without it (the special functions in their switch made them spill).
// Kernels reach it through cost_value_of<COST> / cost_deriv_of<COST> below, and for_cost_link sends Beta under ANY link to a
// COST = PLS_COST_BETA instantiation.
struct BetaLogit {
  double e, mu_s, mu_b, a_s, a_b;
  bool pos;
};
__device__ __forceinline__ BetaLogit beta_logit_reduce(double phi, double f) {
#pragma clang fp contract(off)
  BetaLogit q;
  q.e = fast_exp(-fabs(f));
  q.mu_b = fast_div_normal(1.0, 1.0 + q.e);  // 1 <= 1 + e <= 2
  q.mu_s = q.e * q.mu_b;
  q.a_s = phi * q.mu_s;
  q.a_b = phi * q.mu_b;
  q.pos = f >= 0.0;
  return q;
}
__device__ __forceinline__ double beta_logit_value(double phi, double log_phi, double z, double f) {
#pragma clang fp contract(off)
  const BetaLogit q = beta_logit_reduce(phi, f);
  const double s = 1.0 + q.e, tail = q.e - (s - 1.0);
  const double log_as = (log_phi - fabs(f)) - fast_log_unit_tail(s, tail);
  double lg = -log_as;
#pragma nounroll
  for (int i = 0; i < 2; ++i) lg += lgamma_pos(i ? q.a_b : q.a_s, i == 0);
  return lg - (q.pos ? q.a_b : q.a_s) * z;
}
__device__ __forceinline__ double beta_logit_deriv(double phi, double z, double f) {
#pragma clang fp contract(off)
  const BetaLogit q = beta_logit_reduce(phi, f);
  double d = 0.0;
#pragma nounroll
  for (int i = 0; i < 2; ++i) {
    const double x = xdigamma_pos(i ? q.a_s : q.a_b);
    d = i ? d - q.mu_b * x : q.mu_s * x;
  }
  return (q.pos ? d : -d) - (q.a_s * q.mu_b) * z;
}
// any other link: the header's two formulas in the clipped p = link(f) (the derivative without the link's slope)
__device__ __forceinline__ double beta_link_value(double phi, double z, double p) {
#pragma clang fp contract(off)
  const double a = phi * p, b = phi * (1.0 - p);
  double lg = 0.0;
#pragma nounroll
  for (int i = 0; i < 2; ++i) lg += lgamma_pos(i ? b : a);
  return lg - a * z;
}
__device__ __forceinline__ double beta_link_deriv(double phi, double z, double p) {
#pragma clang fp contract(off)
  double d = -z;
#pragma nounroll
  for (int i = 0; i < 2; ++i) {
    const double x = digamma_pos(i ? phi * (1.0 - p) : phi * p);
    d = i ? d - x : d + x;
  }
  return phi * d;
}

// The ordinal cost (cumulative logit / proportional odds, plship.h) under the identity link.  y holds the category index
// 0 .. 4, p0 .. p3 the ascending cutpoints (+inf for the unused trailing ones); b_0 = -inf and b_5 = +inf complete them, and
// label k lies between lo = b_k and hi = b_(k+1):
//   cost  = softplus(f - hi) + softplus(lo - f),   softplus(t) = max(t, 0) + log1p(e^-|t|)
//   cost' = sigma(f - hi) - sigma(lo - f),   sigma(|t|) = 1 / (1 + e^-|t|),   sigma(-|t|) = e^-|t| / (1 + e^-|t|)
// One exponential per term, the reduction of the negative binomial (nb_exp_reduce); a term with an infinite cutpoint on its own
// side (the top category's upper, the bottom category's lower term) is exactly 0, whatever f is.  lo = +inf (a label >= K) gives
// the value +inf and the derivative -1; a y that is not one of 0 .. 4 selects NaN cutpoints, and the result is that NaN.
// (lo, hi) come from compares of y against 0 .. 4: scalar work where y is uniform across the wave (the row-walking epilogues).
// A kernel that asks for value and derivative calls both functions with the same arguments: the two reductions are the same
// expressions in both and are evaluated once.  Like the Beta code this is NOT a case of cost_value / cost_deriv.
struct OrdinalCuts {
  double lo, hi;
};
__device__ __forceinline__ OrdinalCuts ordinal_cuts(const CostP &c, double y) {
  // (one select per line on values already in registers: a nested ?: chain over the loads of c.p0 .. c.p3 becomes control flow
  // whose merges value and derivative do not share, and then they do not share the exponentials either)
  const double p0 = c.p0, p1 = c.p1, p2 = c.p2, p3 = c.p3, inf = __builtin_huge_val();
  const bool y0 = y == 0.0, y1 = y == 1.0, y2 = y == 2.0, y3 = y == 3.0, y4 = y == 4.0;
  OrdinalCuts k;
  k.lo = __builtin_nan("");
  k.lo = y4 ? p3 : k.lo;
  k.lo = y3 ? p2 : k.lo;
  k.lo = y2 ? p1 : k.lo;
  k.lo = y1 ? p0 : k.lo;
  k.lo = y0 ? -inf : k.lo;
  k.hi = __builtin_nan("");
  k.hi = y4 ? inf : k.hi;
  k.hi = y3 ? p3 : k.hi;
  k.hi = y2 ? p2 : k.hi;
  k.hi = y1 ? p1 : k.hi;
  k.hi = y0 ? p0 : k.hi;
  return k;
}
__device__ __forceinline__ double ordinal_value(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  const OrdinalCuts k = ordinal_cuts(c, y);
  const double tu = f - k.hi, td = k.lo - f;
  const NbExp u = nb_exp_reduce(tu), d = nb_exp_reduce(td);
  const double lu = fast_log_unit_tail(u.s, u.tail), ld = fast_log_unit_tail(d.s, d.tail);  // log1p(e^-|t|) in [0, log 2]
  double up = u.pos ? tu + lu : lu, dn = d.pos ? td + ld : ld;  // softplus(f - hi), softplus(lo - f)
  up = (k.hi == __builtin_huge_val()) ? 0.0 : up;
  dn = (k.lo == -__builtin_huge_val()) ? 0.0 : dn;
  const double v = up + dn;
  return (k.hi == k.hi) ? v : k.hi;
}
__device__ __forceinline__ double ordinal_deriv(const CostP &c, double y, double f) {  // one value for both modes
#pragma clang fp contract(off)
  const OrdinalCuts k = ordinal_cuts(c, y);
  const double tu = f - k.hi, td = k.lo - f;
  const NbExp u = nb_exp_reduce(tu), d = nb_exp_reduce(td);
  const double bu = fast_div_normal(1.0, u.s), bd = fast_div_normal(1.0, d.s);  // sigma(|t|); 1 <= s <= 2
  double a = u.pos ? bu : u.e * bu, b = d.pos ? bd : d.e * bd;  // sigma(f - hi), sigma(lo - f)
  a = (k.hi == __builtin_huge_val()) ? -0.0 : a;  // (-0: an underflowed sigma(lo - f) then leaves -0, the sign of the derivative)
  b = (k.lo == -__builtin_huge_val()) ? -0.0 : b;
  const double g = a - b;
  return (k.hi == k.hi) ? g : k.hi;
}

// The Gamma cost (shape k = p0, mean e^f; plship.h) under the exponential link.  y holds z = log of the observation.  In
// t = z - f:
//   cost  = k (e^t - t)   >= k,      cost' = k (1 - e^t) = -k expm1(t)   in (-inf, k)
// One exponential, no logarithm and no division: fast_exp_expm1 gives e^t and expm1(t) from one reduction, so the derivative is
// relatively accurate at its root t = 0 (the posterior mode), where 1 - e^t would leave an absolute 2^-53.
// t itself rounds where z and f differ in size (at |t| = 600 half an ulp of t is 2^-44: hundreds of ulps of e^t).  A two-sum
// recovers the subtraction's error t_lo exactly, and it enters to first order (t_lo^2 < 2^-88):
//   e^t = e^t_hi (1 + t_lo),   expm1(t) = expm1(t_hi) + e^t_hi t_lo,   e^t - t = (e^t - t_hi) - t_lo
// so value and derivative are a few ulps from the ones at the exact real z - f wherever they are finite.  The ends: e^t_hi = +inf
// (t above the exponential's range, f = -inf, z = +inf) gives the value +inf -- not inf - inf -- and the derivative -inf; where
// e^t underflows the value is -k t and the derivative exactly k (also for z = -inf, an observation of 0, and f = +inf: value
// +inf); a NaN in z or f comes back.  There is one formula for both derivative modes and no clip.
// A kernel that asks for value and derivative calls both functions with the same arguments: the two-sum and the reduction are
// the same expressions in both and are evaluated once.  Like the Beta and ordinal code this is NOT a case of cost_value /
// cost_deriv.
struct GammaT {
  double hi, lo;
};
__device__ __forceinline__ GammaT gamma_t(double z, double f) {
#pragma clang fp contract(off)
  GammaT t;
  t.hi = z - f;
  const double fv = t.hi - z;  // the part of -f that arrived in hi
  const double lo = (z - (t.hi - fv)) + (-f - fv);  // exact: z - f = hi + lo
  t.lo = (fabs(t.hi) < 1024.0) ? lo : 0.0;  // (beyond: e^t is 0 or +inf, and an infinite or NaN hi would leave NaN here)
  return t;
}
__device__ __forceinline__ double gamma_exp_value(const CostP &c, double z, double f) {
#pragma clang fp contract(off)
  const GammaT t = gamma_t(z, f);
  const ExpPair q = fast_exp_expm1(t.hi);
  const double e = fma(q.e, t.lo, q.e);
  double v = (e - t.hi) - t.lo;
  v = (q.e == __builtin_huge_val()) ? q.e : v;
  return c.p0 * v;
}
__device__ __forceinline__ double gamma_exp_deriv(const CostP &c, double z, double f) {  // one value for both modes
#pragma clang fp contract(off)
  const GammaT t = gamma_t(z, f);
  const ExpPair q = fast_exp_expm1(t.hi);
  double em1 = fma(q.e, t.lo, q.em1);
  em1 = (q.e == __builtin_huge_val()) ? q.e : em1;
  return -c.p0 * em1;
}

// cost(y, f) for one (n, j) entry; summed over n by the callers.
__device__ inline double cost_value(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  double slope;
  double p = link_eval(c.link, f, c.jitter, &slope);
  switch (c.cost) {
    case PLS_COST_GAUSSIAN: {  // gaussian.py:63-73 (observation_noise is a variance here)
      double e = p - y;
      return e * e / (2.0 * c.p0);
    }
    case PLS_COST_POISSON:  // poisson.py:59-66
      return -2.0 * y * fast_log(fabs(f)) + p;
    case PLS_COST_BERNOULLI:  // bernoulli.py:57-62
      // binary labels (the usual case) need ONE logarithm; the other term of the general formula is +-0 * finite
      // (p is clipped away from 0 and 1), so these returns are bit-identical to it.  In the row-walking epilogues y
      // is uniform across the wave, so the branch really skips the second log.
      // (one select, ONE logarithm for any mix of the two labels among the lanes of a wave: in the fused small-rank kernels
      // a register holds four different data rows, and `if (y == 1) ... if (y == 0) ...` evaluated both logarithms whenever
      // the four rows did not carry the same label)
      // (with a positive jitter p and 1 - p lie in [jitter, 1 - jitter]: the logarithm without its three special cases)
      if (y == 1.0 || y == 0.0) {
        const double a = (y == 1.0) ? p : 1.0 - p;
        return (c.jitter > 0.0 && c.jitter < 0.5) ? -fast_log_unit(a) : -fast_log(a);
      }
      return -fast_log(p) * y - fast_log(1.0 - p) * (1.0 - y);
    case PLS_COST_STUDENT_T: {  // student_t.py:57-72, p0 = dof, p1 = scale
      double e = p - y;
      return 0.5 * (c.p0 + 1.0) * fast_log(1.0 + e * e / (c.p0 * c.p1 * c.p1));
    }
    case PLS_COST_MULTIMODAL: {  // multimodal.py:37-77, p0 = sigma (std), p1 = shift, p2 = bernoulli_noise
      double e1 = y - p + c.p1, e2 = y - p;
      double a1 = c.mm_l1 - 0.5 * e1 * e1 * c.mm_is2 - c.mm_norm;
      double a2 = c.mm_l2 - 0.5 * e2 * e2 * c.mm_is2 - c.mm_norm;
      double m = fmax(a1, a2);
      return -(m + fast_log(fast_exp(a1 - m) + fast_exp(a2 - m)));
    }
    case PLS_COST_NEGATIVE_BINOMIAL: {  // not in the reference (plship.h): p0 = r, mu = p
      if (c.link == PLS_LINK_EXP) return nb_exp_value(c, y, f);
      const double a = c.p0 * log1p_pos(p * c.ip0);
      return (y == 0.0) ? a : a + y * log1p_pos(fast_div(c.p0, p));
    }
    default:  // (the host entries refuse every other id)
      return __builtin_nan("");
  }
}

// d cost / d f for one entry.
__device__ inline double cost_deriv(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  double slope;
  double p = link_eval(c.link, f, c.jitter, &slope);
  const bool ref = (c.mode == PLS_DERIV_REFERENCE);
  switch (c.cost) {
    case PLS_COST_GAUSSIAN:  // gaussian.py:86-88 closed form == chain rule for the identity link
      return (p - y) * c.ip0 * slope;  // (* 1/sigma2 instead of / sigma2: <= 1 ulp, and no fp64 division per element)
    case PLS_COST_POISSON: {  // poisson.py:76-82 (square link closed form == chain rule); else autograd value
      const double d = fast_div(-2.0 * y, f) + slope;
      // at the pole f = +-0 the closed form divides by f (-+inf, NaN for y = 0); autograd differentiates |f| with
      // sgn(0) = 0 and returns inf * 0
      return (f != 0.0 || (ref && c.link == PLS_LINK_SQUARE)) ? d : __builtin_nan("");
    }
    case PLS_COST_BERNOULLI:
      if (ref && c.link == PLS_LINK_SIGMOID)  // bernoulli.py:64-77, uses the CLIPPED p
        return -y * (1.0 - p) + (1.0 - y) * p;
      return (fast_div(-y, p) + fast_div(1.0 - y, 1.0 - p)) * slope;
    case PLS_COST_STUDENT_T: {  // student_t.py:82-88
      double e = p - y;
      return fast_div((c.p0 + 1.0) * e, c.p0 * c.p1 * c.p1 + e * e) * slope;
    }
    case PLS_COST_MULTIMODAL: {  // multimodal.py:79-91: always the autograd value
      double e1 = y - p + c.p1, e2 = y - p;
      double a1 = c.mm_l1 - 0.5 * e1 * e1 * c.mm_is2;
      double a2 = c.mm_l2 - 0.5 * e2 * e2 * c.mm_is2;
      double m = fmax(a1, a2);
      double w1 = fast_exp(a1 - m), w2 = fast_exp(a2 - m);
      return -fast_div(w1 * e1 + w2 * e2, w1 + w2) * c.mm_is2 * slope;
    }
    case PLS_COST_NEGATIVE_BINOMIAL:  // one value for both modes: there is no reference closed form to tell them apart
      if (c.link == PLS_LINK_EXP) return nb_exp_deriv(c, y, f);
      return fast_div(c.p0 * (p - y), p * (c.p0 + p)) * slope;
    default:  // (the host entries refuse every other id)
      return __builtin_nan("");
  }
}

// The per-element calls of the kernels that are instantiated per pair: COST as for_cost_link passed it (a kernel with
// COST >= 0 sets c.cost = COST, and c.link = LINK where LINK >= 0).  Beta: p0 = phi, y = logit of the observation.  Gamma (only
// ever under the exponential link): p0 = k, y = log of the observation.
__device__ __forceinline__ double beta_cost_value(const CostP &c, double y, double f) {
#pragma clang fp contract(off)
  if (c.link == PLS_LINK_SIGMOID) return beta_logit_value(c.p0, c.mm_l1, y, f);  // (in f: no clip)
  double slope;
  const double p = link_eval(c.link, f, c.jitter, &slope);
  return beta_link_value(c.p0, y, p);
}
__device__ __forceinline__ double beta_cost_deriv(const CostP &c, double y, double f) {  // one value for both modes
#pragma clang fp contract(off)
  if (c.link == PLS_LINK_SIGMOID) return beta_logit_deriv(c.p0, y, f);  // (in f: no clip)
  double slope;
  const double p = link_eval(c.link, f, c.jitter, &slope);
  return beta_link_deriv(c.p0, y, p) * slope;
}
template <int COST>
__device__ __forceinline__ double cost_value_of(const CostP &c, double y, double f) {
  if constexpr (COST == PLS_COST_BETA) return beta_cost_value(c, y, f);
  else if constexpr (COST == PLS_COST_ORDINAL) return ordinal_value(c, y, f);
  else if constexpr (COST == PLS_COST_GAMMA) return gamma_exp_value(c, y, f);
  else return cost_value(c, y, f);
}
template <int COST>
__device__ __forceinline__ double cost_deriv_of(const CostP &c, double y, double f) {
  if constexpr (COST == PLS_COST_BETA) return beta_cost_deriv(c, y, f);
  else if constexpr (COST == PLS_COST_ORDINAL) return ordinal_deriv(c, y, f);
  else if constexpr (COST == PLS_COST_GAMMA) return gamma_exp_deriv(c, y, f);
  else return cost_deriv(c, y, f);
}

}  // namespace plship
