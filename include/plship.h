/*
 * plship.h -- C ABI of libplship.so: the MI355X (gfx950) projected-Langevin-sampling hot path.
 *
 * The reference (jswu18/projected-langevin-sampling) is pure Python/torch and has no FFI; its
 * boundary for this path is the Python plugin API (PLS / PLSBasis / PLSCost / PLSLinkFunction).
 * The entry points below are what a ctypes binding for that API calls.  Each one cites the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every array pointer is a DEVICE pointer to float64 unless the name ends in _host;
 *   - matrices are row-major with an explicit leading dimension (elements, not bytes);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued asynchronously, nothing synchronises, nothing allocates (callers hand in
 *     workspaces), so every call may be captured into a hipGraph;
 *   - return value: 0 = PLS_OK, otherwise a pls_status; pls_last_error() returns a
 *     thread-local human readable message for the last failing call on this thread;
 *   - no global mutable state: descriptor structs are plain data owned by the caller, the
 *     library is thread-compatible (different threads may call with different streams).
 *
 * N = training points, M = inducing points, Mk = kept eigen-directions (<= M), J = particles
 * (columns; a rank may own a J-shard and pass its global column offset), D = input dim.
 */
#ifndef PLSHIP_H
#define PLSHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLSHIP_ABI_VERSION 7

typedef enum {
  PLS_OK = 0,
  PLS_ERR_INVALID_ARGUMENT = 1,
  PLS_ERR_HIP = 2,
  PLS_ERR_WORKSPACE_TOO_SMALL = 3,
  PLS_ERR_UNSUPPORTED = 4
} pls_status;

/* base kernel k (third party gpytorch ScaleKernel(RBFKernel(ard)) in the reference,
 * constructed at experiments/uci/regression/main.py:171-173; MockKernel = mockers/kernel.py:13-23).
 * MATERN12 / 32 / 52: gpytorch ScaleKernel(MaternKernel(nu = 1/2, 3/2, 5/2)) with ARD lengthscales (since ABI 7):
 * with r = |(a - b) / lengthscale| and t = sqrt(2 nu) r,  k = outputscale * p(t) * exp(-t),  p = 1, 1 + t, 1 + t + t^2/3.
 * RQ: gpytorch ScaleKernel(RQKernel) with ARD lengthscales and the shape parameter alpha > 0.  An addition within ABI 7 (no
 * existing signature, struct or value changes; a build has it where pls_gp_mll_workspace_bytes_kind is exported); its value
 * is 6, because 5 stays the value that every entry refuses as unknown.  With
 * r^2 = sum_k ((a_k - b_k) / lengthscale_k)^2 and u = r^2 / (2 alpha),  k = outputscale * kappa,  kappa = (1 + u)^-alpha =
 * exp(-alpha log1p(u)).  For this kind EVERY `lengthscale` argument of this header points to d + 1 doubles: the d
 * lengthscales, then alpha (pls_gp_mll_grad_classes: d + 1 per class).  kappa is exactly 1 at distance 0; an entry is
 * exactly 0 where alpha log1p(u) > 745.2 or 1 + u overflows (r = inf included), which only a large alpha brings about.
 *   d kappa / d log lengthscale_k = kappa / (1 + u) ((a_k - b_k) / lengthscale_k)^2
 *   d kappa / d log alpha         = alpha kappa (u / (1 + u) - log1p(u))                    (exactly 0 at distance 0)
 * PERIODIC: gpytorch ScaleKernel(PeriodicKernel(ard_num_dims = d)) AS RECALLED -- a reading of its documentation, not a run of
 * gpytorch; the formula here is the contract and it is what the tests hold.  An addition within ABI 7 (no export is added or
 * changed); its value is 8, because 5 and 7 stay values that every entry refuses as unknown.  With lengthscales lambda_k > 0
 * (they DIVIDE and are not squared: MacKay's l^2 is this lambda), period lengths p_k > 0 and e_k = (a_k - b_k) / p_k:
 *   kappa                  = exp(-2 sum_k sin^2(pi e_k) / lambda_k),      k = outputscale * kappa
 *   dk / d log lambda_k    = outputscale * kappa * 2 sin^2(pi e_k) / lambda_k
 *   dk / d log p_k         = outputscale * kappa * (2 / lambda_k) * pi e_k * sin(2 pi e_k)
 * For this kind EVERY `lengthscale` argument of this header points to 2 d doubles: the d lengthscales, then the d period
 * lengths (pls_gp_mll_grad_classes: 2 d per class), and 1 <= d <= 16 (the other kinds: 64); the workspace queries return 0
 * for d > 16.  Evaluation, the same in the Gram build, the gradient reduction, the fused mean and the selector: the
 * difference first, e_k = (a_k - b_k) * (1 / p_k), r = e - rint(e) with |r| <= 1/2, sin(pi r) and cos(pi r) from the
 * library's own polynomials (about 1 ulp; sin(pi 0) = 0 exactly), sin(2 pi e) = 2 sin cos of that evaluation, e itself in
 * front of the period term, the terms of the exponent added in ascending k.  So kappa is exactly 1 at distance 0 and for
 * any pair an exact whole number of periods apart (a power-of-two period makes e exact), k is exactly symmetric, and k
 * does not change by a bit under a translation of all points that is exact in fp64.  A pair whose exponent is below -745.2
 * is exactly 0 and skipped in every sum.  The kernel has NO limit at infinity: a non-finite difference gives NaN.
 * LOCALLY_PERIODIC: gpytorch ScaleKernel(RBFKernel(ard_num_dims = d) * PeriodicKernel(ard_num_dims = d)) AS RECALLED, the
 * locally periodic (quasi-periodic) kernel -- a reading, not a run of gpytorch; the formula here is the contract and it is what
 * the tests hold.  An addition within ABI 7 (no export is added or changed); its value is 10, because 9 stays a value that
 * every entry refuses as unknown, like 5 and 7.  With envelope lengthscales l_k > 0, periodic lengthscales lambda_k > 0 (they
 * divide and are not squared, as PERIODIC's), period lengths p_k > 0 and e_k = (a_k - b_k) / p_k, the two factors share one
 * exponential:
 *   kappa                  = exp(-(1/2 sum_k ((a_k - b_k) / l_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k)),   k = outputscale * kappa
 *   dk / d log l_k         = outputscale * kappa * ((a_k - b_k) / l_k)^2
 *   dk / d log lambda_k    = outputscale * kappa * (2 / lambda_k) sin^2(pi e_k)
 *   dk / d log p_k         = outputscale * kappa * (2 / lambda_k) * pi e_k * sin(2 pi e_k)
 * For this kind EVERY `lengthscale` argument of this header points to 3 d doubles: the d envelope lengthscales l_k, then the
 * d periodic lengthscales lambda_k, then the d period lengths p_k (pls_gp_mll_grad_classes: 3 d per class), and
 * 1 <= d <= 16, PERIODIC's limit; the workspace queries return 0 for d > 16.  The reduction returns 3 d + 1 sums in the order
 * kappa, l, lambda, p, and an evaluation 4 + 3 d outputs.  Evaluation, the same in the Gram build, the gradient reduction, the
 * fused mean and the selector: the points are not pre-scaled; per coordinate the difference first, then z = (a_k - b_k) *
 * (1 / l_k) and PERIODIC's evaluation of (2 / lambda_k) sin^2(pi e_k); the coordinate's two shares are added first, in one
 * fused multiply-add (z / 2) * z + (2 / lambda_k) sin^2(pi e_k), then the coordinates in ascending k; ONE exponential of the
 * negated sum.  So kappa is exactly 1 at distance 0, k is exactly symmetric, and k does not change by a bit under a
 * translation of all points that is exact in fp64.  A pair whose exponent is below -745.2 is exactly 0 and skipped in every
 * sum.  A non-finite difference gives NaN.  NOT guaranteed, unlike PERIODIC: kappa = 1 a whole number of periods apart -- the
 * envelope forbids it.
 * TREND_SEASONAL: gpytorch ScaleKernel(RBFKernel(ard_num_dims = d)) + ScaleKernel(RBFKernel(ard_num_dims = d) *
 * PeriodicKernel(ard_num_dims = d)) AS RECALLED, a slow trend ADDED to a locally periodic seasonal part -- a reading, not a run
 * of gpytorch; the formula here is the contract and it is what the tests hold.  An addition within ABI 7 (no export is added
 * or changed); its value is 12, because 11 stays a value that every entry refuses as unknown, like 5, 7 and 9.  The sum is ONE
 * kind whose second outputscale is a shape value.  With trend lengthscales l_k > 0, the seasonal term's envelope lengthscales
 * m_k > 0, periodic lengthscales lambda_k > 0 (they divide and are not squared), period lengths p_k > 0, e_k = (a_k - b_k) / p_k,
 * the trend outputscale s_t (the `outputscale` argument of every entry) and the seasonal outputscale s_s > 0:
 *   kappa_t = exp(-1/2 sum_k ((a_k - b_k) / l_k)^2)
 *   kappa_s = exp(-(1/2 sum_k ((a_k - b_k) / m_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k))          (LOCALLY_PERIODIC's kappa)
 *   k                      = s_t * kappa_t + s_s * kappa_s
 *   dk / d log l_k         = s_t * kappa_t * ((a_k - b_k) / l_k)^2
 *   dk / d log m_k, d log lambda_k, d log p_k = LOCALLY_PERIODIC's three, with s_s * kappa_s in front
 *   dk / d log s_s         = s_s * kappa_s
 * For this kind EVERY `lengthscale` argument of this header points to 4 d + 1 doubles: the d trend lengthscales l_k, then the d
 * envelope lengthscales m_k, then the d periodic lengthscales lambda_k, then the d period lengths p_k, then s_s
 * (pls_gp_mll_grad_classes: 4 d + 1 per class), and 1 <= d <= 8: the reduction carries 4 d + 2 accumulators per thread, at 8
 * fewer than LOCALLY_PERIODIC carries at 16.  A larger d is refused ("> 8 is not supported for the trend-plus-seasonal
 * kernel") and the workspace queries return 0 for it.  The reduction returns 4 d + 2 sums in the order kappa_t, l, m, lambda,
 * p, s_s, and an evaluation 4 + 4 d + 1 outputs.  Evaluation, the same in the Gram build, the gradient reduction, the fused
 * mean and the selector: the points are not pre-scaled; per coordinate the difference first; the seasonal term is
 * LOCALLY_PERIODIC's evaluation with (m, lambda, p), bit for bit; the trend's distance sum takes the same difference times
 * (1 / l_k), squared and accumulated by fused multiply-add in ascending k, and one exponential of minus half of it.  Each
 * term takes its own underflow decision: a term whose exponent is below -745.2 is exactly 0 and skipped in every sum.  The
 * entry is fma(s_t, kappa_t, s_s * kappa_s): k(x, x) is s_t + s_s rounded once, a pair with a dead trend has exactly
 * LOCALLY_PERIODIC's entry for (m, lambda, p, s_s), a pair with a dead seasonal term exactly s_t * kappa_t.  k is exactly
 * symmetric and does not change by a bit under a translation of all points that is exact in fp64.  A non-finite difference
 * gives NaN. */
typedef enum {
  PLS_KERNEL_RBF_ARD = 0,
  PLS_KERNEL_LINEAR = 1,
  PLS_KERNEL_MATERN12 = 2,
  PLS_KERNEL_MATERN32 = 3,
  PLS_KERNEL_MATERN52 = 4,
  PLS_KERNEL_RQ = 6, /* (5 is not a kind) */
  PLS_KERNEL_PERIODIC = 8, /* (7 is not a kind) */
  PLS_KERNEL_LOCALLY_PERIODIC = 10, /* (9 is not a kind) */
  PLS_KERNEL_TREND_SEASONAL = 12    /* (11 is not a kind) */
} pls_kernel_kind;

/* src/projected_langevin_sampling/costs/{gaussian,poisson,bernoulli,student_t,multimodal}.py
 * NEGATIVE_BINOMIAL is not in the reference: an addition within ABI 7 (no export is added or changed), for over-dispersed
 * counts.  p[0] = r, the dispersion, 0 < r < inf; mean mu = link(f), variance mu + mu^2 / r.  The value is the negative
 * log-likelihood WITHOUT its f-independent terms (so energies are comparable between runs with the same r only):
 *   cost(y, f)      = r log1p(mu / r) + y log1p(r / mu)                 (the second term is exactly 0 for y == 0)
 *   d cost / d f    = r (mu - y) / (mu (r + mu)) * d mu / d f
 * y >= 0 need not be an integer.  Both derivative modes return the same bits: there is no reference closed form to tell
 * them apart.  Under PLS_LINK_EXP, with t = f - log r (log r taken on the host), mu is never formed:
 *   cost(y, f)      = r softplus(t) + y softplus(-t),    softplus(+-t) = max(+-t, 0) + log1p(exp(-|t|))
 *   d cost / d f    = r sigma(t) - y sigma(-t)           in [-y, r]
 * so value and derivative are finite where exp(f) overflows or underflows (about r t for large t, about -y t for large -t).
 * This pair has kernel instantiations of its own on every step route; under any other link the formulas in mu are evaluated
 * by the chain rule.
 * BETA is not in the reference either (an addition within ABI 7), for proportions in (0, 1).  Mean-precision form:
 * mu = link(f), a = phi mu, b = phi (1 - mu), p[0] = phi, the precision, 0 < phi < inf.  The library's y argument holds
 * z_n = logit(y_n) = log y_n - log1p(-y_n), NOT y_n: any finite z is valid (a proportion next to 0 or 1 keeps its bits).
 * The value is the negative log-likelihood WITHOUT its f-independent terms lgamma(phi), log y, phi log(1 - y) (so energies
 * are comparable between runs with the same phi only):
 *   cost(z, f)      = lgamma(a) + lgamma(b) - a z
 *   d cost / d f    = phi [psi(a) - psi(b) - z] * d mu / d f
 * Both derivative modes return the same bits.  Under PLS_LINK_SIGMOID the pair is evaluated in f without the link's clip
 * (the jitter is ignored, as EXP ignores it).  With e = exp(-|f|), mu_s = e / (1 + e), mu_b = 1 / (1 + e), a_s = phi mu_s,
 * a_b = phi mu_b, w = phi mu_s mu_b, X(x) = x psi(x) (= -1 + x psi(1 + x) for small x) and sg = sign(f) (+1 at +-0):
 *   cost(z, f)      = [lgamma(1 + a_s) - (log phi - |f| - log1p(e))] + lgamma(a_b) - (f >= 0 ? a_b : a_s) z
 *   d cost / d f    = sg (w psi(a_b) - mu_b X(a_s)) - w z
 * The bracket is lgamma(a_s) with log a_s formed from its parts, finite where a_s underflows; X(a_s) -> -1 keeps the
 * derivative finite in the tails: it tends to +-1 as f -> +-inf (exactly +-1 at f = +-1e300), a bounded drift.  This pair
 * has kernel instantiations of its own on every step route; under any other link the first two formulas are evaluated in
 * the clipped p = link(f) by the chain rule.
 * ORDINAL is not in the reference either (an addition within ABI 7), for ordered categories 0 .. K-1, 2 <= K <= 5: the
 * cumulative-logit (proportional-odds) model P(y <= k | f) = sigma(b_(k+1) - f).  p[0..3] hold the cutpoints b_1 < b_2 < ...
 * in ascending order, the unused trailing entries +inf, so K = 1 + the number of finite entries; p[0] is finite.  b_0 = -inf
 * and b_K = +inf.  The library's y argument holds the category index as a double.  For label k write lo = b_k, hi = b_(k+1).
 * The value is the negative log-likelihood WITHOUT its f-independent term -log(1 - exp(-(hi - lo))) (so energies are
 * comparable between runs with the same cutpoints only):
 *   cost(k, f)      = softplus(f - hi) + softplus(lo - f),    softplus(t) = max(t, 0) + log1p(exp(-|t|))
 *   d cost / d f    = sigma(f - hi) - sigma(lo - f)           in (-1, 1)
 * with sigma(|t|) = 1 / (1 + exp(-|t|)), sigma(-|t|) = exp(-|t|) / (1 + exp(-|t|)): each term is evaluated in t = f - cutpoint
 * with one exponential.  The top category's upper term and the bottom category's lower term (an infinite cutpoint on its own
 * side) are exactly 0.  Both derivative modes return the same bits; the jitter is ignored.  A y that is not one of 0, 1, 2,
 * 3, 4 (NaN included) gives NaN for value and derivative; a label >= K (its lower cutpoint is +inf) gives the value +inf and
 * the derivative -1: callers validate their labels.  Only PLS_LINK_IDENTITY is accepted (ordered probit is not provided);
 * the pair has kernel instantiations of its own on every step route.
 * GAMMA is not in the reference either (an addition within ABI 7), for strictly positive, right-skewed continuous data.
 * p[0] = k, the shape (concentration), 0 < k < inf; mean mu = exp(f), variance mu^2 / k.  The library's y argument holds
 * z_n = log y_n, NOT y_n: any finite z is valid (an observation beyond the fp64 range of y keeps its bits).  With t = z - f
 * the value is the negative log-likelihood WITHOUT its f-independent terms z + lgamma(k) - k log k (so energies are
 * comparable between runs with the same k only):
 *   cost(z, f)      = k (exp(t) - t)                      >= k, = k at f = log y
 *   d cost / d f    = k (1 - exp(t)) = -k expm1(t)        in (-inf, k)
 * exp(t) and expm1(t) come from one argument reduction; the derivative is relatively accurate at its root t = 0.  The rounding
 * of the subtraction z - f is recovered (a two-sum) and applied to first order, so value and derivative are within a few ulps
 * of the ones at the exact real z - f wherever they are finite.  The edges:
 *   t above the exponential's range (e^t rounds to +inf), f = -inf or z = +inf:   value +inf (never NaN), derivative -inf
 *   e^t underflows:                                                                value -k t, derivative exactly k
 *   z = -inf (y = 0) or f = +inf:                                                  value +inf, derivative k
 *   a NaN in z or f:                                                               that NaN, in value and derivative
 * (z and f infinite with the same sign have no difference: NaN; finite z and f whose fp64 difference overflows count as
 * t = +-inf).  Both derivative modes return the same bits, and the jitter is ignored.  Only PLS_LINK_EXP is accepted; the pair
 * has kernel instantiations of its own on every step route.  The drift is bounded above by k but not below, and its slope in f
 * is k e^t: the stable step size behaves like Poisson's (it shrinks with the largest y_n / mu_n a particle meets), not like
 * that of the three bounded families NEGATIVE_BINOMIAL/EXP, BETA/SIGMOID and ORDINAL. */
typedef enum {
  PLS_COST_GAUSSIAN = 0,
  PLS_COST_POISSON = 1,
  PLS_COST_BERNOULLI = 2,
  PLS_COST_STUDENT_T = 3,
  PLS_COST_MULTIMODAL = 4,
  PLS_COST_NEGATIVE_BINOMIAL = 5,
  PLS_COST_BETA = 7, /* (6 is not a kind) */
  PLS_COST_ORDINAL = 9, /* (8 is not a kind) */
  PLS_COST_GAMMA = 11  /* (10 is not a kind) */
} pls_cost_kind;

/* src/projected_langevin_sampling/link_functions.py:30-80
 * EXP is not in the reference (an addition within ABI 7): p = exp(f), slope p, no clip -- the jitter is ignored; +inf above
 * the fp64 range, gradual underflow below it.  Under a cost other than NEGATIVE_BINOMIAL and GAMMA (which is stated in f
 * itself) it runs by the generic chain rule. */
typedef enum {
  PLS_LINK_IDENTITY = 0,
  PLS_LINK_SQUARE = 1,
  PLS_LINK_SIGMOID = 2,
  PLS_LINK_PROBIT = 3,
  PLS_LINK_EXP = 4
} pls_link_kind;

/* How d cost / d f is evaluated.
 *   PLS_DERIV_REFERENCE: what the reference's calculate_cost_derivative dispatch does -- the closed
 *     form when (cost, link) is one of its matched pairs (gaussian.py:103-106, poisson.py:97-100,
 *     bernoulli.py:92-95, student_t.py:103-106), otherwise the autograd value.
 *   PLS_DERIV_AUTOGRAD: the value costs/base.py:68-84 (vmap(jacfwd)) returns, evaluated analytically
 *     by the chain rule (clip has zero slope outside its range), for every (cost, link) pair. */
typedef enum { PLS_DERIV_REFERENCE = 0, PLS_DERIV_AUTOGRAD = 1 } pls_deriv_mode;

typedef struct {
  int32_t cost;       /* pls_cost_kind */
  int32_t link;       /* pls_link_kind */
  int32_t deriv_mode; /* pls_deriv_mode */
  int32_t reserved;
  /* p[0..3]: gaussian {observation_noise (a VARIANCE, gaussian.py:71,86)};
   *          student_t {degrees_of_freedom, scale};
   *          multimodal {observation_noise (a STD, multimodal.py:56), shift, bernoulli_noise};
   *          negative_binomial {dispersion r};
   *          beta {precision phi};
   *          ordinal {up to four ascending cutpoints, +inf for the unused trailing ones};
   *          gamma {shape k};
   *          poisson / bernoulli: unused */
  double p[4];
  double jitter; /* clip of sigmoid / probit links (link_functions.py:36, :64), default 1e-10 */
} pls_cost_desc;

/* Langevin noise source for one step. */
typedef enum {
  PLS_NOISE_NONE = 0,     /* drift only (tests) */
  PLS_NOISE_INJECTED = 1, /* xi is read from memory: parity runs inject the oracle's noise */
  PLS_NOISE_PHILOX = 2    /* in-kernel Philox4x32-10 + Box-Muller, counter = (row, global column, step) */
} pls_noise_kind;

typedef struct {
  int32_t kind; /* pls_noise_kind */
  int32_t reserved;
  const double *xi; /* PLS_NOISE_INJECTED: (rows x J) standard-normal matrix */
  int64_t ldxi;
  uint64_t seed;    /* PLS_NOISE_PHILOX */
  uint64_t step;    /* PLS_NOISE_PHILOX: step counter, so every step draws fresh noise */
  int64_t j_offset; /* global index of local column 0 (J-sharding: results do not depend on the GPU count) */
  /* PLS_NOISE_PHILOX, optional: a DEVICE counter read at run time; the step used is *step_base + step.  Launch arguments
   * are frozen into a captured hipGraph, this word is not: a graph of K steps (step = 0..K-1) followed by
   * pls_counter_add(step_base, K) draws fresh noise on every replay. */
  const uint64_t *step_base;
} pls_noise_desc;

/* Orthonormal basis state (reference: basis/orthonormal.py:22-68), produced by the setup calls below.
 *   A  = V~^T k(Z,X)      (Mk x N), lda   -- V~ = V diag(1/sqrt(Mk*lambda)) (orthonormal.py:63-68)
 *   At = k(X,Z) V~        (N x Mk), ldat  -- the same matrix transposed, so both contractions stream
 *                                            k-major operands (DESIGN.md "data layout")
 *   lam = kept eigenvalues of k(Z,Z)/M (Mk)
 * Optional Gaussian/identity fast path (paper's O(M^3 + J M^2) step): B = A A^T (Mk x Mk), c = A y (Mk entries,
 * followed by ONE more entry c[Mk] = y^T y used by the fast energy). */
typedef struct {
  int64_t mk, n;
  const double *A;
  int64_t lda;
  const double *At;
  int64_t ldat;
  const double *lam;
  const double *B; /* may be NULL */
  int64_t ldb;
  const double *c; /* may be NULL */
} pls_onb_desc;

/* Cholesky factor of an SPD matrix K = Lc Lc^T as pls_chol_factor leaves it on the device:
 *   Lc  (M x M, lower, row-major) and LcT = Lc^T (upper): the same factor stored both ways, so that either is a k-major
 *       operand of the MFMA contraction;
 *   Sf, Sb (M x M): the block forward / backward substitution operators.  With D_b the inverse of the b-th 128 x 128
 *       DIAGONAL block of Lc:  Sf[k][i] = -(D_b Lc[b, k-block])^T for k-blocks left of block b (i in block b), D_b^T on the
 *       diagonal block;  Sb[k][i] = -(Lc[k-block, b] D_b) for k-blocks below, D_b on the diagonal.  One block row of a
 *       solve is then a single MFMA k-loop; K^-1 itself is never formed.  NULL if the factor is only used for L xi. */
typedef struct {
  int64_t m;
  const double *Lc;
  int64_t ldlc;
  const double *LcT;
  int64_t ldlct;
  const double *Sf;
  int64_t ldsf;
  const double *Sb;
  int64_t ldsb;
  /* Optional (ABI 3): the inverse factor Linv = Lc^-1 (M x M, lower, row-major) and its transpose LinvT, as
   * pls_chol_build_inverse leaves them (column c of Lc^-1 by forward substitution of e_c).  With them a solve is one
   * (forward) or two (forward + backward) TRIANGULAR PRODUCTS on the MFMA contraction instead of a block substitution:
   * any number of right-hand sides fills the chip, which the substitution -- a workgroup per 32 columns, serial over the
   * block rows -- does not on the narrow J-shard of an 8-GPU run.  NULL: block substitution only. */
  const double *Linv;
  int64_t ldlinv;
  const double *LinvT;
  int64_t ldlinvt;
  /* Optional (ABI 4): scratch for BALANCED triangular products on few output tiles (pls_tri_scratch_bytes(M, J) bytes,
   * 16-byte aligned).  A triangular operand gives tile row t of a product a contraction of (t + 1) * 64 rows; when every
   * workgroup is resident at once (M = 1024, J = 1024: 256 tiles on 256 CUs) the launch lasts as long as its heaviest tile,
   * i.e. as long as the full product.  With the scratch, tile rows t and nti - 1 - t are shared by two workgroups with equal
   * loads; the heavy tile's two partial sums meet through a scratch slot and are added by whichever workgroup arrives
   * second (deterministic: a + b == b + a; nobody waits).  Contract: the first 16 KB (flag words) are ZERO when the scratch
   * is first handed in; every call leaves them zero; calls that may run concurrently (different streams) need different
   * scratches.  NULL: one tile per workgroup. */
  void *tri_scratch;
  size_t tri_scratch_bytes;
} pls_chol_desc;

/* Inducing-point basis state (reference: basis/inducing_point.py:23-50).
 *   Kzx = k(Z,X) (M x N), Kxz = its transpose (N x M);
 *   k(Z,Z) enters through its Cholesky factor (pls_chol_factor): LcT = Lc^T for the noise colouring e = Lc xi, and the
 *   substitution operators Sf / Sb for the two solves per step, V = k(Z,Z)^-1 U = Lc^-T Lc^-1 U (the reference's
 *   gpytorch.solve, inducing_point.py:89-93, :130-132).
 *   W = k(Z,Z)^-1 (M x M, symmetric) is OPTIONAL and only used for A/B runs: with Sf/Sb == NULL, or after
 *   pls_set_option(PLS_OPT_IPB_EXPLICIT_INVERSE, 1), the solves are replaced by the contraction W U. */
typedef struct {
  int64_t m, n;
  const double *Kzx;
  int64_t ldkzx;
  const double *Kxz;
  int64_t ldkxz;
  const double *W; /* may be NULL when Sf / Sb are set */
  int64_t ldw;
  const double *LcT; /* may be NULL when noise is injected already coloured */
  int64_t ldlct;
  const double *B; /* optional Gaussian fast path: Kzx Kxz (M x M), see pls_ipb_build_gaussian */
  int64_t ldb;
  const double *c; /* optional: Kzx y (M), then y^T y */
  const double *Sf; /* substitution operators of pls_chol_factor (see pls_chol_desc) */
  int64_t ldsf;
  const double *Sb;
  int64_t ldsb;
  /* Optional (ABI 3): the inverse factor of k(Z,Z) (see pls_chol_desc) ... */
  const double *Linv;
  int64_t ldlinv;
  const double *LinvT;
  int64_t ldlinvt;
  /* ... and the Gaussian/identity operator in WHITENED coordinates S = Lc^-1 U (pls_ipb_build_whitened, built for ONE
   * observation noise: q_inv_noise = 1 / sigma2):  Q = Lc^-1 (B / sigma2 + M I) Lc^-T (M x M), ct = Lc^-1 c / sigma2 (M entries,
   * then y^T y).  With them pls_ipb_step's Gaussian path is forward solve + Q S (fused update kernel) + Lc dS, and
   * pls_ipb_whitened_step advances S itself with ONE M x M x J contraction per step. */
  const double *Q;
  int64_t ldq;
  const double *ct;
  double q_inv_noise;
  /* Optional (ABI 4): scratch for balanced triangular products (see pls_chol_desc.tri_scratch): the forward solve and the
   * product with Lc of pls_ipb_step's whitened route, pls_ipb_whiten / _unwhiten, the solves of the other routes. */
  void *tri_scratch;
  size_t tri_scratch_bytes;
  /* Optional (ABI 4): Pt = Lc^-T Q (M x M; pls_ipb_build_step_operator), the whitened operator with the forward solve folded
   * in: Q S = Q Lc^-1 U = P U, so pls_ipb_step computes dS from U itself and a call is TWO launches (P U with the fused
   * update + noise, then Lc dS) and 3 M^2 J flop instead of three and 4 M^2 J.  Built for the same observation noise as
   * Q (q_inv_noise).  A call that asks for energy_in keeps the three-launch route (the energy is a quadratic form in S). */
  const double *Pt;
  int64_t ldpt;
  /* Optional (ABI 5): Awa ((n + m) x m, k-major like Kxz, 16-byte aligned rows, even ldawa; pls_ipb_build_whitened_operand),
   * the forward operand of WHITENED particles with the prior as rows: rows [0, n) = k(X,Z) Lc^-T (F = Awa S for S = Lc^-1 U),
   * rows [n, n + m) = sqrt(m) Lc^-T, whose "cost" is f^2 / 2 -- their back-projection is the prior drift m (Lc^T Lc)^-1 S and
   * their cost the prior energy (m / 2) |k(Z,Z)^-1 U|^2.  With it the step of a cost without the Gaussian algebra in whitened
   * coordinates is the one-launch small-rank step and nothing else (pls_ipb_whitened_generic_step). */
  const double *Awa;
  int64_t ldawa;
} pls_ipb_desc;

/* Step-size search (experiments/runners.py:331-446): the S candidate step sizes run as S column blocks of ONE particle
 * matrix, block b = columns [b * block_cols, (b + 1) * block_cols).  Every block is an independent copy of the same
 * sampler: its step size is eta[b], and its noise stream is the one a stand-alone run of block_cols particles would
 * draw (Philox column = j_offset + column inside the block), so a batched search reproduces the sequential one.
 * eta is a DEVICE array: a block whose search has ended is frozen by writing 0 (update and noise both vanish). */
typedef struct {
  int64_t block_cols;
  const double *eta; /* device, cdiv(j, block_cols) entries */
  /* Optional output (ABI 3), steps with energy_in != NULL only: cdiv(j, 256) doubles, entry i = the sum of the per-particle
   * energies of columns [256 i, 256 (i + 1)) in the library's fixed order (pls_chunk_sums).  On the Gaussian/identity fast
   * paths the launch that finishes the energy by-product writes them (no second launch per training iteration); every
   * other route appends one pls_chunk_sums launch, so the field is honoured whatever the descriptor and the options
   * select.  The mean energy of a block of columns that starts at a multiple of 256 is then a few host additions over
   * these entries (ascending order: the value pls_block_means returns, bit for bit).  May point to pinned host memory
   * mapped into the device.  NULL: not written. */
  double *energy_sums;
  /* Optional (ABI 4), Gaussian/identity fast paths with energy_in != NULL: cdiv(j, 256) 32-bit counters (device), ZERO when
   * first handed in; every call leaves them zero.  With them the step launch FINISHES the energies itself -- the workgroup
   * that arrives last at a 256-column chunk adds the partial rows of that chunk in their fixed order, writes energy_in and
   * energy_sums (the values the finishing launch computes, bit for bit) -- so a training iteration is ONE launch.  Calls
   * that may run concurrently need different counters.  NULL (or any other route): a finishing launch follows. */
  uint32_t *energy_sync;
  /* Optional (ABI 4), LAGGED energies for training loops on the Gaussian/identity fast paths (pls_onb_step_blocks,
   * pls_ipb_whitened_step_blocks).  The reduction of a step's energy by-product over the tile rows is a global dependency
   * behind its last MFMA: finished inside the launch it adds 4.4-5 us of serial tail, as a launch of its own 6-9 us.  Instead:
   *   energy_partials       (out) this launch leaves ONLY its partial rows here (pls_energy_partials_bytes(rows, j) bytes;
   *                         energy_in / energy_sums / energy_sync are then not used);
   *   energy_partials_prev  (in)  the partial rows the PREVIOUS launch of the loop left (another buffer: alternate two); this
   *                         launch finishes them at its START, under the landing of its first operand rows, into
   *   energy_prev           (out) the J energies of the previous launch's input particles, and
   *   energy_sums_prev      (out, optional) their 256-column chunk sums (may be pinned host memory);
   *   energy_flush          1: no step at all -- the last launch's partial rows are finished by a small launch of their own
   *                         (pass the particle matrix and step arguments of the step calls; out may be NULL).
   * The values are the ones the other forms compute, bit for bit; they arrive one launch later. */
  double *energy_partials;
  const double *energy_partials_prev;
  double *energy_prev;
  double *energy_sums_prev;
  int32_t energy_flush;
  int32_t reserved;
  /* Optional (ABI 5), orthonormal basis with at most 128 functions and a cost without the Gaussian algebra, problems in the
   * launch-bound regime (the sizes of the reference's own experiments: N, J in the hundreds to thousands): the whole
   * step -- projection, cost derivative, back-projection, the fixed-order sum over the row slabs, prior drift, noise, and with
   * energy_in the energies of the input particles and their energy_sums -- is ONE launch (csrc/small_rank_step.h; option
   * PLS_OPT_SMALL_RANK_STEP).  Its workgroups meet through pls_step_sync_words(j) 32-bit counters: handed in here they must
   * be ZERO when first handed in and every call leaves them zero (calls that may run concurrently need different
   * counters); NULL: the launch is preceded by a memset node over counters carved from the workspace. */
  uint32_t *step_sync;
  /* Optional output (ABI 5), steps with energy_in != NULL only: cdiv(j, 16) doubles, entry b = the sum of the per-particle
   * energies of columns [16 b, 16 (b + 1)) added in ascending column order.  The one-launch step writes them for free (the
   * workgroup that finishes a column block holds its sixteen energies), where energy_sums costs it a second hand-over
   * between workgroups; every other route appends one small launch.  A training loop adds the entries in ascending order
   * on the host.  May point to pinned host memory mapped into the device.  NULL: not written. */
  double *energy_sums16;
} pls_block_desc;

const char *pls_last_error(void);
int pls_abi_version(void);

/* Route options (the defaults are what bench.py measures; tests flip them to reach both code paths).  NOTHING here is
 * process-wide: every option is a value of the CALLING THREAD (each thread starts from the defaults), and a launch takes the
 * routes of the thread that makes the call -- two bases driven from two host threads can choose differently, and a test
 * that flips an option disturbs no other thread.  (The per-launch timeline of pls_timeline_begin / _end and the text behind
 * pls_last_error are per thread as well.)
 *   PLS_OPT_SMALL_RANK_MAX: bases with at most this many functions (0..128, default 128) take the fused small-rank
 *   kernels (F, d cost / d f and the back-projection in ONE pass: the N x J matrices F and G are never written);
 *   larger ranks, or 0, take the two-GEMM path.  Results agree to rounding, not bit for bit. */
typedef enum pls_option {
  PLS_OPT_SMALL_RANK_MAX = 1,
  /* 1: V = k(Z,Z)^-1 U of the inducing-point basis as the contraction W U with the explicit inverse (needs
   * pls_ipb_desc.W); 0 (default): two blocked triangular solves with the Cholesky factor (pls_chol_solve). */
  PLS_OPT_IPB_EXPLICIT_INVERSE = 2,
  /* Contractions with few output tiles (a narrow J-shard of an 8-GPU run: Mk x Mk x J/8) take 64 x 64 tiles whose k range
   * is split over two wave groups INSIDE the workgroup (csrc/gemm_tn_f64_kg.h), so that 256..1023 tiles still put 2..4
   * waves on every SIMD; the epilogue runs once on the fixed-order sum.  MODE: 0 off, 1 automatic (default), 2 / 3 force the
   * two- / one-group kernel wherever the operands are 16-byte aligned (A/B runs, tests).  MAX_TILES: the number of
   * 128 x 128 output tiles below which the automatic mode takes it (default 256: one workgroup per CU). */
  PLS_OPT_KSPLIT_MODE = 3,
  PLS_OPT_KSPLIT_MAX_TILES = 4,
  /* Solves with the Cholesky factor of k(Z,Z): 1 (default) = triangular products with the inverse factor wherever the
   * descriptor carries Linv / LinvT, 0 = block substitution (tri_solve_strip_kernel) always. */
  PLS_OPT_SOLVE_MODE = 5,
  /* (6, 7: the wave-pair fused kernel for 129 .. 256 functions of ABI 3; slower than the row-block back-projection at every
   * rank and removed in ABI 4) */
  /* Back-projection D = A G of a basis whose function count is above 128 and not a multiple of 128 (two-GEMM path):
   * 1 (default) = one launch of csrc/gemm_tn_f64_rows.h (equal-height tiles, the MFMA count follows the rank in steps of
   * 16, G read once); 0 = 128-row tiles plus 64- / 32- / 16-row remainder launches (round 2). */
  PLS_OPT_ROW_BLOCKS = 8,
  /* Triangular products on few output tiles with a scratch in the descriptor (pls_chol_desc.tri_scratch): 1 (default) =
   * balanced (csrc/gemm_tn_f64_kg.h, gemm_tn_f64_kg_tri_kernel), 0 = one tile per workgroup (A/B runs, tests). */
  PLS_OPT_TRI_BALANCE = 9,
  /* pls_ipb_step, Gaussian/identity without energy_in: 1 (default) = dS = -eta (P U - ct) + noise straight from U when the
   * descriptor carries Pt, 0 = forward solve, then Q S (A/B runs, tests). */
  PLS_OPT_IPB_STEP_OPERATOR = 10,
  /* 1 (default): pls_block_desc.energy_sync is honoured (the step launch finishes the energies); 0: always a finishing
   * launch (A/B runs, tests). */
  PLS_OPT_ENERGY_FUSED_FINISH = 11,
  /* 1 (default): the k-split kernel of narrow particle shards draws the Philox noise of its output block in front of its
   * k-loop, while the first operand rows travel; 0: in the epilogue, like the other tilings.  Same bits either way. */
  PLS_OPT_KG_NOISE_PREGEN = 12,
  /* Steps of the orthonormal basis with at most 128 functions and a cost without the Gaussian algebra: 1 (default) = ONE
   * launch (csrc/small_rank_step.h) while the problem is launch-bound (at most 4096 particles and 8 GFLOP per step), the
   * slab kernels of csrc/small_rank.h + update launch beyond; 0 = never; 2 = wherever the kernel applies (A/B runs, tests).
   * Results agree to rounding (another summation order over the data rows), not bit for bit. */
  PLS_OPT_SMALL_RANK_STEP = 13,
  /* pls_ipb_step on at most 128 inducing points, in front of the one-launch step above: 1 (default) = V = k(Z,Z)^-1 U and the
   * coloured Philox noise Lc xi in ONE launch (csrc/ipb_prep.h; needs the inverse factor Linv / LinvT in the descriptor and
   * PLS_OPT_SOLVE_MODE 1), 0 = the two triangular products, the fill and the third product as launches of their own (A/B
   * runs, tests).  Same draws either way; results agree to rounding. */
  PLS_OPT_IPB_PREP = 14,
  /* The general step of the orthonormal basis through pls_onb_step_wg / pls_onb_step_blocks_wg with the basis' left-hand
   * planes (pls_onb_winograd_prepare): 1 (default) = one level of Strassen-Winograd for the back-projection D = A G where J is
   * a multiple of 128 and >= 2048 and the workspace holds the route's layout in chunks of >= 8192 paired rows: seven half-size
   * products instead of eight, 7/8 of the matrix work of the back-projection (csrc/winograd.h); 0 = the
   * plain contraction (A/B runs, tests).  Deterministic either way; results agree to rounding, not bit for bit. */
  PLS_OPT_WINOGRAD = 15
} pls_option;
/* Diagnostic: out[i] = op(x[i]) with the device exp (op 0) / log (op 1) the per-element kernels use (csrc/fmath.h), or
 * out[i] = x[i] / x[n + i] with their division (op 2: fast_div, IEEE special cases restored; op 3: fast_div_normal), so
 * that their accuracy can be pinned against libm; op 4: lgamma(x), op 5: digamma(x), op 6: x digamma(x), for x > 0, as the
 * Beta cost evaluates them (csrc/special_device.h).  Not on the step path. */
int pls_debug_math(int32_t op, const double *x, double *out, int64_t n, void *stream);
int pls_set_option(int32_t option, int64_t value);
int64_t pls_get_option(int32_t option); /* -1 for an unknown option */

/* Per-launch timeline (measurement only; off by default, zero cost when off).  Between begin and end, every
 * kernel the calling thread launches through this library is bracketed by two HIP events recorded on the
 * launch's own stream.  pls_timeline_end synchronises on them and returns, per launch, its duration in
 * milliseconds and a pls_kernel_tag; it returns the number of launches seen (<= capacity recorded). */
typedef enum {
  PLS_TAG_GEMM_STORE = 1,            /* gemm_tn_f64, plain / accumulate epilogue (back-projection A G, setup GEMMs) */
  PLS_TAG_GEMM_COST_DERIV = 2,       /* gemm_tn_f64, F tile -> d cost / d f epilogue */
  PLS_TAG_GEMM_COST_VALUE = 3,       /* gemm_tn_f64, F tile -> per-column cost partial sums */
  PLS_TAG_GEMM_LANGEVIN_GAUSSIAN = 4,/* gemm_tn_f64, B U with the whole Langevin update in the epilogue */
  PLS_TAG_LANGEVIN_UPDATE = 5,
  PLS_TAG_KERNEL_GRAM = 6,
  PLS_TAG_OTHER = 7,
  PLS_TAG_SMALL_RANK_DRIFT = 8,      /* small_rank_kernel: F, d cost / d f and the back-projection in one pass (rank <= 128) */
  PLS_TAG_SMALL_RANK_VALUE = 9,      /* small_rank_kernel: F and the per-column cost sums in one pass */
  PLS_TAG_TRI_SOLVE = 10,            /* tri_solve_strip_kernel: V = Lc^-T Lc^-1 U, forward + backward substitution in one launch */
  PLS_TAG_SMALL_RANK_STEP = 11,      /* small_rank_step_kernel: the whole step (and its energies) of a small-rank basis in one launch */
  PLS_TAG_IPB_PREP = 12              /* ipb_prep_kernel: V = k(Z,Z)^-1 U and the coloured noise Lc xi of a step, <= 128 inducing points */
} pls_kernel_tag;
int pls_timeline_begin(int32_t capacity);
int pls_timeline_end(float *ms, int32_t *tags, int32_t capacity, int32_t *count);

/* ---------------------------------------------------------------------------------------------
 * Primitive operators (un-fused entry points; a user-defined Python cost or basis composes these)
 * ------------------------------------------------------------------------------------------- */

/* out(n1 x n2) = k(x1, x2); x1 (n1 x d), x2 (n2 x d) row-major contiguous.
 * Replaces kernel.base_kernel(x1=.., x2=..) at orthonormal.py:36-41, inducing_point.py:41-46.
 * lengthscale: d values (every kind except LINEAR needs it; ignored for LINEAR); RQ: d + 1, alpha last; LOCALLY_PERIODIC: 3 d (l, lambda, p; d <= 16); TREND_SEASONAL: 4 d + 1 (l, m, lambda, p, s_s; d <= 8); PERIODIC: 2 d, the
 * period lengths behind the lengthscales, and d <= 16. */
int pls_kernel_gram(int32_t kernel_kind, const double *x1, int64_t n1, const double *x2, int64_t n2,
                    int64_t d, const double *lengthscale, double outputscale, double *out, int64_t ldout,
                    void *stream);

/* Leading dimensions.  Every ld* argument and descriptor field counts doubles and is an int64_t; a strided view of a
 * wider buffer is a valid operand.  The element-wise and reduction kernels index with 64 bits and take ANY leading
 * dimension: pls_kernel_gram, pls_cost_derivative, pls_cost_value, pls_link_transform, pls_row_power_sums,
 * pls_row_quantiles, pls_normal_fill, pls_softmax_normal_mean, pls_kernel_mean, pls_sym_eigh, pls_svgp_*, pls_gp_mll_*,
 * pls_onb_build_gaussian, pls_ipb_build_gaussian, pls_chol_factor's K, and the output / particle / noise arguments
 * (ldu, ldo, ldf, ldg, ldxi) of every step, forward, update and energy entry wherever they are not an operand of a
 * contraction.  The MFMA kernels address operands with 32-bit byte offsets behind 2 GiB buffer descriptors.  For each
 * such site the call is either ROUTED to a kernel that takes the stride (nothing to do for the caller) or REFUSED with
 * PLS_ERR_INVALID_ARGUMENT and a message that names the leading dimension -- never answered with wrong numbers:
 *   - contraction operands (ldl, ldr of pls_gemm_tn; lda, ldat, ldb of pls_onb_desc; ldkzx, ldkxz, ldw, ldlct, ldb,
 *     ldlinv, ldlinvt, ldq, ldpt, ldawa of pls_ipb_desc; the particles U / S where a step contracts them; ldvs, ldkzx of
 *     pls_onb_build_projection; ldlc, ldlct, ldsf, ldsb of pls_chol_factor and pls_chol_build_operators): a shape of
 *     few tiles runs on the k-split kernels while both leading dimensions are below 2^22, and is ROUTED to the tile
 *     kernels from 2^22 on.  The 128 x 128 tiles (256 or more of them), their row-block form and the Winograd route
 *     copy 16-byte aligned operands with even leading dimensions by LDS-DMA and REFUSE ld >
 *     pls_ld_limit(PLS_LD_GEMM_TILES, 1, cols) = (0x7FFFFFF0 - 8 cols) / 120 for an operand of `cols` columns, an odd
 *     count rounded up to even (17895688 at cols = 128).  Operands that are not so
 *     aligned, and every shape below 256 tiles of 128 x 128, load through 64-bit pointers: no limit.
 *   - contraction outputs (ldc of pls_gemm_tn, ldf of pls_onb_forward / pls_ipb_forward, the outputs of the Gaussian
 *     fast-path steps, the outputs of the solves' products): interior tiles are stored from registers below 2^21 and
 *     through LDS with 64-bit addresses from 2^21 on (ROUTED inside the kernel): no limit.
 *   - the substitution kernel (pls_chol_solve, pls_chol_build_inverse; pls_chol_forward_solve and pls_chol_solve_ws
 *     when they substitute; the solves inside the pls_ipb_* entries): ldu, ldv REFUSED above
 *     pls_ld_limit(PLS_LD_TRI_SOLVE, m, j) = (0x7FFFFF00 / 8 - j) / (min(m, 128) - 1), and ldsf, ldsb above the same
 *     with j = m (2113664 at m >= 128, j = 96).
 *   - the fused small-rank kernels and the one-launch step (mk or m <= 128): ROUTED to the contraction kernels when the
 *     back-projection operand's leading dimension (ldat, ldkxz) exceeds pls_ld_limit(PLS_LD_SMALL_RANK, ..) = 2^23;
 *     pls_ipb_whitened_generic_step, which has no other kernel, REFUSES ldawa beyond it (pls_ipb_whitened_generic_applies
 *     returns 0 for such a descriptor).
 *   - the solve-and-noise launch of the inducing-point step (m <= 128): ROUTED to the separate solve and noise launches
 *     when ldlinv, ldlinvt or ldlct exceeds pls_ld_limit(PLS_LD_IPB_PREP, m, 1) = (0x7FFFFFF0 / 8 - m) / (m - 1).
 * pls_ld_limit returns the largest leading dimension a site takes (the bound the library itself applies; pure host
 * code; -1 for an unknown site or rows / cols < 1). */
typedef enum {
  PLS_LD_GEMM_TILES = 0,        /* LDS-DMA k-loop of the 128 x 128 tiles: operand of `cols` columns (refused beyond) */
  PLS_LD_GEMM_KSPLIT = 1,       /* k-split kernels (routed to the tile kernels beyond) */
  PLS_LD_GEMM_DIRECT_STORE = 2, /* register -> global tile store (routed through LDS beyond) */
  PLS_LD_TRI_SOLVE = 3,         /* substitution kernel: factor of order `rows`, operand of `cols` columns (refused beyond) */
  PLS_LD_SMALL_RANK = 4,        /* fused small-rank kernels (routed to the contraction kernels beyond) */
  PLS_LD_IPB_PREP = 5           /* solve-and-noise launch: factor of order `rows` (routed to separate launches beyond) */
} pls_ld_site;
int64_t pls_ld_limit(int32_t site, int64_t rows, int64_t cols);

/* C(I x J) = alpha * L^T R + beta * C with L (K x I, ldl), R (K x J, ldr): the fp64 MFMA contraction.
 * Replaces every `@` on the path: orthonormal.py:106-108, :152-155; inducing_point.py:89-93, :144.
 * Leading dimensions: ldl, ldr as contraction operands, ldc as a contraction output (above). */
int pls_gemm_tn(const double *L, int64_t ldl, const double *R, int64_t ldr, double *C, int64_t ldc, int64_t I,
                int64_t J, int64_t K, double alpha, double beta, void *stream);

/* The kernel pls_gemm_tn would launch for these arguments under the calling thread's options, decided by the launchers'
 * own predicates; nothing is launched and L, R are only inspected for alignment.  *direct_store (may be NULL): 1 when
 * interior tiles are stored from registers, 0 when every tile leaves through LDS.  Returns a pls_gemm_route, or
 * -PLS_ERR_INVALID_ARGUMENT when pls_gemm_tn would refuse the call (pls_last_error() says why).  I, J >= 1. */
typedef enum {
  PLS_GEMM_ROUTE_TILES_128 = 0,
  PLS_GEMM_ROUTE_TILES_64 = 1,
  PLS_GEMM_ROUTE_KSPLIT_1 = 2,
  PLS_GEMM_ROUTE_KSPLIT_2 = 3,
  PLS_GEMM_ROUTE_ROW_BLOCKS = 4
} pls_gemm_route;
int pls_gemm_tn_route(const double *L, int64_t ldl, const double *R, int64_t ldr, int64_t ldc, int64_t I, int64_t J,
                      int64_t K, int32_t *direct_store);

/* Which fused small-rank kernels the step and energy entries would hand the back-projection operand Lb (n x kdim, ldlb:
 * At of pls_onb_desc, Kxz or Awa of pls_ipb_desc) for targets y and j particle columns, under the calling thread's
 * options, by the entries' own predicates; nothing is launched and Lb, y are only inspected for alignment.  Returns an
 * OR of pls_small_rank_route_bits (0: the contraction kernels take the operand), or -PLS_ERR_INVALID_ARGUMENT.
 * Leading dimensions: ldlb as the small-rank kernels' operand (above): both bits clear beyond 2^23. */
typedef enum {
  PLS_SMALL_RANK_SLABS = 1,     /* the slab kernels of the general routes and energies (kdim <= PLS_OPT_SMALL_RANK_MAX) */
  PLS_SMALL_RANK_ONE_LAUNCH = 2 /* the one-launch step (PLS_OPT_SMALL_RANK_STEP, 16-byte aligned y, launch-bound sizes) */
} pls_small_rank_route_bits;
int pls_small_rank_route(const double *Lb, int64_t ldlb, int64_t kdim, int64_t n, const double *y, int64_t j);

/* G(N x J) = d cost / d f evaluated at F(N x J), y(N).  Replaces PLSCost.calculate_cost_derivative
 * (costs/gaussian.py:86-88, poisson.py:76-82, bernoulli.py:64-77, student_t.py:82-88, base.py:68-84).
 * Leading dimensions: ldf, ldg any (64-bit indexing). */
int pls_cost_derivative(const pls_cost_desc *cost, const double *F, int64_t ldf, const double *y, int64_t n,
                        int64_t j, double *G, int64_t ldg, void *stream);

/* c(J) = sum_n cost(y_n, F_nj).  Replaces PLSCost.calculate_cost (gaussian.py:63-73, poisson.py:59-66,
 * bernoulli.py:57-62, student_t.py:57-72, multimodal.py:37-77).  Deterministic summation order.
 * workspace: pls_cost_value_workspace_bytes(n, j) bytes.  Leading dimensions: ldf any (64-bit indexing). */
size_t pls_cost_value_workspace_bytes(int64_t n, int64_t j);
int pls_cost_value(const pls_cost_desc *cost, const double *F, int64_t ldf, const double *y, int64_t n, int64_t j,
                   double *c, void *workspace, size_t workspace_bytes, void *stream);

/* out = link(in + col_offset[col]) element-wise (rows x cols); col_offset may be NULL.
 * Replaces PLSLinkFunction.transform (link_functions.py:30-80) and, with the per-particle observation noise as
 * col_offset, PLSCost.predict_samples (costs/base.py:117-133). */
int pls_link_transform(int32_t link, double jitter, const double *in, int64_t ldin, int64_t rows, int64_t cols,
                       const double *col_offset, double *out, int64_t ldout, void *stream);

/* out[r] = sum_j (S[r][j] - shift[r])^power, power in {1, 2}, shift may be NULL; fixed summation order.
 * The two passes (power 1 -> mean, power 2 about the mean) replace prediction_samples.mean(dim=1) / .var(axis=1) at
 * costs/gaussian.py:49-52; on a J-sharded run each pass is followed by one all-reduce of `rows` doubles. */
int pls_row_power_sums(const double *S, int64_t lds, int64_t rows, int64_t cols, const double *shift, int32_t power,
                       double *out, void *stream);

/* out[r][k] = q[k]-quantile of row r of S (rows x cols), linear interpolation between order statistics at position
 * q * (cols - 1): the value torch.quantile(S, q, dim=1) returns (conformalise/pls.py:36-45, :57-62).  Up to 16384
 * samples per row one workgroup sorts the row in LDS (bitonic); longer rows (a large calibration split, the gathered
 * samples of a J-sharded run) take a radix selection of the two order statistics instead (nine passes over the row, no
 * workspace).  q: nq values in [0, 1] (device).  A row that contains a NaN yields NaN, like torch. */
int pls_row_quantiles(const double *S, int64_t lds, int64_t rows, int64_t cols, const double *q, int32_t nq, double *out,
                      int64_t ldout, void *stream);

/* *counter += increment on the stream (device word; see pls_noise_desc.step_base). */
int pls_counter_add(uint64_t *counter, uint64_t increment, void *stream);

/* out(rows x J) standard normals from the library's counter-based generator (same stream the fused
 * step uses).  Replaces torch.normal at basis/base.py:55-63 and samplers.py:30-35 for on-device runs. */
int pls_normal_fill(double *out, int64_t ldout, int64_t rows, int64_t j, uint64_t seed, uint64_t step,
                    int64_t j_offset, void *stream);

/* out[b] = mean of e[b * block_cols .. (b + 1) * block_cols) (the last block may be shorter), b < nblocks; fixed
 * summation order.  Replaces `.mean()` of the per-particle energies (orthonormal.py:126, inducing_point.py:115), per
 * step-size candidate when the particle matrix holds several (pls_block_desc).  `out` may be device memory or pinned
 * host memory mapped into the device (the training loop reads it after an event, without a copy kernel). */
int pls_block_means(const double *e, int64_t j, int64_t block_cols, double *out, void *stream);

/* out[i] = sum of e[256 i .. min(j, 256 (i + 1))): the chunk sums every energy mean of the library is built from (xor
 * butterfly inside each wave, then (w0 + w1) + (w2 + w3); pls_block_means adds the chunks of a block in ascending order). */
int pls_chunk_sums(const double *e, int64_t j, double *out, void *stream);

/* Cholesky factorisation on the device: K (M x M, SPD, row-major; only read) + jitter * I = Lc Lc^T.
 * Replaces the factorisation inside gpytorch.solve(lhs = k(Z,Z), ...) (inducing_point.py:89-93, :104-106, :130-132,
 * :235-239) and the per-step eigh(k(Z,Z)) of the noise sampler (samplers.py:27 via inducing_point.py:133-137).
 * Right-looking blocked algorithm, 64-column panels; the trailing updates run on the fp64 MFMA contraction.
 * Outputs (caller-allocated, M x M each, 16-byte aligned, even leading dimensions): Lc, LcT and -- unless NULL -- the
 * substitution operators Sf, Sb (see pls_chol_desc).  info (DEVICE int32): 0, or the 1-based index of the first
 * pivot that was not positive (K + jitter I is not numerically positive definite; the outputs are then garbage and the
 * caller retries with a larger jitter, as gpytorch's psd_safe_cholesky does).  Nothing synchronises.
 * Leading dimensions: ldk any (64-bit indexing); ldlc, ldlct, ldsf, ldsb as contraction operands and outputs (above). */
int pls_chol_factor(const double *K, int64_t ldk, int64_t m, double jitter, double *Lc, int64_t ldlc, double *LcT,
                    int64_t ldlct, double *Sf, int64_t ldsf, double *Sb, int64_t ldsb, int32_t *info, void *stream);

/* The substitution operators Sf, Sb (see pls_chol_desc) of a factor that is already on the device -- pls_chol_factor
 * ends with this call; parity runs upload the oracle's own LAPACK factor (Lc and its transpose, zeros in the other
 * triangle) and build the operators from it, so that both sides solve with the SAME factor.  Sf and Sb must be zero
 * outside the blocks this call writes (block upper / lower triangle).
 * Leading dimensions: ldlc, ldlct, ldsf, ldsb as contraction operands and outputs (above; the solves that later read Sf,
 * Sb have the substitution kernel's limit). */
int pls_chol_build_operators(const double *Lc, int64_t ldlc, const double *LcT, int64_t ldlct, int64_t m, double *Sf,
                             int64_t ldsf, double *Sb, int64_t ldsb, void *stream);

/* V (M x J) = K^-1 U = Lc^-T Lc^-1 U: block forward then backward substitution in ONE launch (a workgroup owns 32
 * columns for the whole solve).  Replaces gpytorch.solve(lhs = k(Z,Z), input = k(Z,Z), rhs = U).  V must not alias U.
 * Leading dimensions: ldu, ldv, ldsf, ldsb as operands of the substitution kernel (refused beyond PLS_LD_TRI_SOLVE). */
int pls_chol_solve(const pls_chol_desc *factor, const double *U, int64_t ldu, int64_t j, double *V, int64_t ldv,
                   void *stream);

/* PLS_OK if the substitution kernel takes a right-hand side and a solution of j >= 1 columns with these leading dimensions
 * and the descriptor's ldsf, ldsb; else the refusal pls_chol_solve (and every entry that substitutes) would answer with.
 * The entries' own check; pure host code, nothing is launched and no pointer is dereferenced. */
int pls_chol_solve_check(const pls_chol_desc *factor, int64_t ldu, int64_t j, int64_t ldv);

/* Linv = Lc^-1 and LinvT = Lc^-T (M x M each, 16-byte aligned, even leading dimensions): the identity pushed through the
 * block forward substitution of pls_chol_solve, column by column the backward-stable solve Lc x = e_c.  Needs Sf / Sb.
 * Leading dimensions: ldlinv, ldlinvt, ldsf, ldsb as operands of the substitution kernel (refused beyond PLS_LD_TRI_SOLVE). */
int pls_chol_build_inverse(const pls_chol_desc *factor, double *Linv, int64_t ldlinv, double *LinvT, int64_t ldlinvt,
                           void *stream);

/* Y (M x J) = Lc^-1 U: the forward half of pls_chol_solve (one triangular product with LinvT when the descriptor has it
 * and PLS_OPT_SOLVE_MODE is 1, block forward substitution otherwise).  Y must not alias U.
 * Leading dimensions: as pls_gemm_tn's (ldlinvt, ldu operands; ldy output) on the product route, as pls_chol_solve's when it
 * substitutes. */
int pls_chol_forward_solve(const pls_chol_desc *factor, const double *U, int64_t ldu, int64_t j, double *Y, int64_t ldy,
                           void *stream);

/* Bytes of pls_chol_desc.tri_scratch / pls_ipb_desc.tri_scratch for products with M rows and up to J columns (16 KB of
 * flag words, then two 32 KB partial-sum slots per pair of 64-row tile rows and 64-column tile). */
size_t pls_tri_scratch_bytes(int64_t m, int64_t j);

/* pls_chol_solve with a workspace of pls_chol_solve_workspace_bytes(M, J): with Linv / LinvT in the descriptor (and
 * PLS_OPT_SOLVE_MODE 1) the solve is two triangular products, Lc^-1 U into the workspace and Lc^-T of that into V; a
 * narrow J-shard then uses every CU (M = 1024, J = 1024: 32 workgroups of the substitution kernel on 256 CUs).
 * Leading dimensions: as pls_gemm_tn's (ldlinv, ldlinvt, ldu operands; ldv output) on the product route, as pls_chol_solve's
 * when it substitutes. */
size_t pls_chol_solve_workspace_bytes(int64_t m, int64_t j);
int pls_chol_solve_ws(const pls_chol_desc *factor, const double *U, int64_t ldu, int64_t j, double *V, int64_t ldv,
                      void *workspace, size_t workspace_bytes, void *stream);

/* out (M x J) = Lc X with the TRANSPOSED factor LcT (upper) as the k-major operand; only k <= row is contracted.
 * Colours standard normals: e = Lc xi ~ N(0, k(Z,Z)) (replaces sample_multivariate_normal's Q sqrt(Lambda) xi,
 * samplers.py:37-44, same law).  Leading dimensions: ldlct, ldx as contraction operands, ldo as a contraction output. */
int pls_tri_multiply(const double *LcT, int64_t ldlct, int64_t m, const double *X, int64_t ldx, int64_t j, double *out,
                     int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exact-GP hyper-parameters: the marginal log-likelihood and its gradient
 * ------------------------------------------------------------------------------------------- */

/* The d + 1 sums over all ordered pairs (i, j) of n points that the gradient of the exact-GP marginal log-likelihood
 * with respect to the base kernel's parameters is made of (the kernel-dependent part of loss.backward() at
 * experiments/trainers.py:49, gpytorch's autograd through ScaleKernel(RBFKernel | MaternKernel)).  With
 * e_k = (x_ik - x_jk) / lengthscale_k, r^2 = sum_k e_k^2, W_ij = alpha_i alpha_j - P_ij and kappa the kernel WITHOUT
 * its outputscale s:
 *   out[0]     = sum_ij W_ij kappa_ij                                   (the d / d log s sum, divided by s)
 *   out[1 + k] = sum_ij W_ij dK_ij / d log lengthscale_k
 *       RBF:    dK_ij / d log l_k = s exp(-r^2 / 2) e_k^2
 *       Matern: dK_ij / d log l_k = s q(t) exp(-t) 2 nu e_k^2,  t = sqrt(2 nu) r,  q = 1/t, 1, (1 + t)/3 (nu = 1/2, 3/2, 5/2)
 *       RQ:     dK_ij / d log l_k = s kappa / (1 + u) e_k^2,  u = r^2 / (2 alpha)
 *       PERIODIC: dK_ij / d log lambda_k = s kappa 2 sin^2(pi e_k) / lambda_k,  e_k = (x_ik - x_jk) / p_k
 *   out[1 + d] = sum_ij W_ij dK_ij / d log alpha = sum_ij W_ij s alpha kappa (u / (1 + u) - log1p(u))          (RQ only)
 *   out[1 + d + k] = sum_ij W_ij dK_ij / d log p_k = sum_ij W_ij s kappa (2 / lambda_k) pi e_k sin(2 pi e_k)   (PERIODIC only)
 *   LOCALLY_PERIODIC (3 d + 1 sums, kappa the product's): out[1 + k] = sum_ij W_ij s kappa ((x_ik - x_jk) / l_k)^2, then
 *       out[1 + d + k] = sum_ij W_ij dK_ij / d log lambda_k and out[1 + 2 d + k] = sum_ij W_ij dK_ij / d log p_k as PERIODIC's two
 *   TREND_SEASONAL (4 d + 2 sums; s = s_t, the `outputscale` argument): out[0] = sum_ij W_ij kappa_t,
 *       out[1 + k] = sum_ij W_ij s_t kappa_t ((x_ik - x_jk) / l_k)^2, out[1 + d + k], out[1 + 2 d + k] and out[1 + 3 d + k]
 *       LOCALLY_PERIODIC's sums for its envelope lengthscale (here m_k), lambda_k and p_k with s_s kappa_s in the place of
 *       s kappa, out[1 + 4 d] = sum_ij W_ij s_s kappa_s = sum_ij W_ij dK_ij / d log s_s; d <= 8, and 0 workspace bytes above
 * A pair with r = 0 (the diagonal, duplicated points) contributes exactly 0 to every out[1 + k]; a pair whose
 * exponential underflows contributes exactly 0 to every sum; a pair with r = 0 contributes exactly 0 to out[1 + d] too.
 * PLS_KERNEL_LINEAR is rejected.
 * x (n x d) row-major contiguous, alpha (n; the solve's vector, not RQ's shape), P (n x n, SYMMETRIC, leading dimension
 * ldp; read once -- 16 bytes per lane where ldp is even and P is 16-byte aligned), out (d + 1, device; RQ: d + 2; LOCALLY_PERIODIC: 3 d + 1; PERIODIC:
 * 2 d + 1).  kappa is
 * recomputed from x; no Gram matrix is read.
 * Deterministic summation order (no atomics): two calls give the same bits.
 * workspace: pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d) = 8 S ceil(n / 512) ceil(n / 64) bytes with S = d + 1
 * sums (RQ: d + 2; PERIODIC: 2 d + 1, LOCALLY_PERIODIC: 3 d + 1, and 0 bytes for d > 16); pls_kernel_grad_sums_workspace_bytes(n, d)
 * is the S = d + 1 value (every kind but RQ, PERIODIC and LOCALLY_PERIODIC). */
size_t pls_kernel_grad_sums_workspace_bytes(int64_t n, int64_t d);
size_t pls_kernel_grad_sums_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d);
int pls_kernel_grad_sums(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                         double outputscale, const double *alpha, const double *P, int64_t ldp,
                         double *out /* d + 1 (RQ: d + 2; PERIODIC: 2 d + 1; LOCALLY_PERIODIC: 3 d + 1), device */, void *workspace, size_t workspace_bytes, void *stream);

/* The exact-GP predictive mean at t test points WITHOUT the n x t cross-Gram matrix: replaces the mean of
 * model(experiment_data.train.x) at experiments/uci/regression/main.py:231 (every subsample GP predicts at all N training
 * points for estimate_student_parameters, :109-125; the variance that gpytorch computes beside it is thrown away there).
 * With kappa the kernel WITHOUT its outputscale s, evaluated entry for entry as pls_kernel_gram evaluates it:
 *   out[i] = mean + s * sum_j kappa(xt_i, x_j; lengthscale) alpha[j]                 i < t,  j < n
 * A pair whose exponential underflows contributes exactly 0; a pair at distance 0 contributes alpha[j] (kappa = 1 for
 * every kind, Matern-1/2 included: 1/t is never formed).  PLS_KERNEL_LINEAR is rejected; d <= 64.
 * x (n x d) and xt (t x d) row-major contiguous, alpha (n), out (t): device memory.  x is read 16 bytes per lane where it
 * is 16-byte aligned, xt where it is 16-byte aligned and d is even; one double per lane otherwise (the same bits).
 * Summation order (no atomics, no workspace): a workgroup owns 64 test points, one per lane; wave w of its four adds
 * the terms of the training points j = w, w + 4, w + 8, ... in ascending order into one accumulator per thread (there
 * is no cross-lane sum, so no butterfly); the four waves' sums are added as (w0 + w1) + (w2 + w3); then
 * out[i] = fma(s, sum, mean) (TREND_SEASONAL: two accumulators per thread, A_t of kappa_t and A_s of kappa_s, each summed
 * that way, and out[i] = fma(s_t, A_t, fma(s_s, A_s, mean))).  The split of j depends on j alone -- not on t, n, d or the position of the point in
 * the batch -- so out[i] is a function of xt_i and the model: a batch can be split anywhere and gives the same bits
 * (as pls_softmax_normal_mean), and two calls give the same bits.
 * t == 0 returns PLS_OK and launches nothing; n >= 1.  Nothing synchronises or allocates. */
int pls_kernel_mean(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                    double outputscale, double mean, const double *alpha, const double *xt, int64_t t,
                    double *out /* t, device */, void *stream);

/* One evaluation of the exact-GP marginal log-likelihood and its gradient: replaces mll(model(x), y) and
 * loss.backward() at experiments/trainers.py:45-49 (gpytorch ExactMarginalLogLikelihood, GaussianLikelihood,
 * ConstantMean, one output).  With K_y = s kappa(x, x) + (noise + jitter) I = Lc Lc^T, r = y - mean, alpha = K_y^-1 r
 * and W = alpha alpha^T - K_y^-1:
 *   out[0]     = mll = -1/2 r^T alpha - sum_i log Lc_ii - n/2 log 2 pi
 *   out[1]     = d mll / d mean  = sum_i alpha_i
 *   out[2]     = d mll / d noise = 1/2 tr W
 *   out[3]     = d mll / d log s
 *   out[4 + k] = d mll / d log lengthscale_k                            (d mll / d theta = 1/2 sum_ij W_ij dK_ij / d theta)
 *   out[4 + d] = d mll / d log alpha                                    (RQ only: its out has 5 + d doubles)
 *   out[4 + d + k] = d mll / d log p_k                                  (PERIODIC only: its out has 4 + 2 d doubles)
 *   LOCALLY_PERIODIC (4 + 3 d doubles): out[4 + k] = d mll / d log l_k, out[4 + d + k] = d mll / d log lambda_k,
 *       out[4 + 2 d + k] = d mll / d log p_k
 *   TREND_SEASONAL (4 + 4 d + 1 doubles, S = 4 d + 2 sums, d <= 8): out[3] = d mll / d log s_t, out[4 + k] = d mll / d log l_k,
 *       out[4 + d + k] = d mll / d log m_k, out[4 + 2 d + k] = d mll / d log lambda_k, out[4 + 3 d + k] = d mll / d log p_k,
 *       out[4 + 4 d] = d mll / d log s_s
 * Steps: pls_kernel_gram, the diagonal, pls_chol_factor, pls_chol_solve, pls_chol_build_inverse, K_y^-1 = Linv^T Linv on
 * the MFMA contraction, pls_kernel_grad_sums with P = K_y^-1, a one-workgroup finishing kernel (fixed-order sums).
 * out: 4 + d doubles (RQ: 5 + d; PERIODIC: 4 + 2 d; LOCALLY_PERIODIC: 4 + 3 d), device memory or pinned host memory mapped into the device.  info (DEVICE int32): as
 * pls_chol_factor -- 0, or the 1-based index of the first pivot that was not positive; the outputs are then unspecified
 * and the caller retries with a larger jitter.  Nothing synchronises or allocates.
 * workspace (16-byte aligned): with ld = n rounded up to even and v(k) = k rounded up to even,
 *   pls_gp_mll_workspace_bytes_kind(kind, n, d) = 8 (7 n ld + 2 v(n) + v(S ceil(n / 512) ceil(n / 64)) + v(S)) bytes:
 * seven n x ld planes (K_y, reused for K_y^-1; Lc; Lc^T; Sf; Sb; Linv, which first holds the Gram matrix; Linv^T), r,
 * alpha, the partial rows of the reduction and its S sums, S = d + 1 (RQ: d + 2; PERIODIC: 2 d + 1, LOCALLY_PERIODIC: 3 d + 1, and 0 bytes for d > 16).
 * pls_gp_mll_workspace_bytes(n, d) is the S = d + 1 value: what every kind but RQ, PERIODIC and LOCALLY_PERIODIC needs.  The entry checks against the kind-aware value. */
size_t pls_gp_mll_workspace_bytes(int64_t n, int64_t d);
size_t pls_gp_mll_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d);
int pls_gp_mll_grad(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                    double outputscale, double noise, double mean, double jitter, const double *y,
                    double *out /* 4 + d (RQ: 5 + d; PERIODIC: 4 + 2 d; LOCALLY_PERIODIC: 4 + 3 d), device or mapped pinned host */, int32_t *info /* device */,
                    void *workspace, size_t workspace_bytes, void *stream);

/* The same evaluation for `classes` independent GPs on the shared x, in ONE call: the per-epoch work of exact-GP
 * classification with gpytorch's DirichletClassificationLikelihood(learn_additional_noise=True) and a batch of
 * num_classes GPs (experiments/curves/classification/main.py:162-192; Milios et al. 2018).  Class c has its own
 * lengthscales, outputscale s_c, constant mean, learned noise sigma_c and a FIXED noise per point:
 *   K_y,c = s_c kappa(x, x; l_c) + diag(fixed_noise[c][.] + noise[c] + jitter)
 * fixed_noise == NULL: no fixed part (row c is then exactly pls_gp_mll_grad with class c's parameters).
 *   lengthscale (classes x d, contiguous; RQ: classes x (d + 1), alpha last in each row; PERIODIC: classes x 2 d; LOCALLY_PERIODIC: classes x 3 d) DEVICE;  outputscale, noise, mean (classes each) HOST arrays, read before the
 *   call returns;  fixed_noise (classes x n, leading dimension ldf) and y (classes x n, leading dimension ldy) DEVICE.
 *   out (classes x (4 + d), RQ: classes x (5 + d), PERIODIC: classes x (4 + 2 d), LOCALLY_PERIODIC: classes x (4 + 3 d), contiguous; device or mapped pinned host): row c laid out as the out of pls_gp_mll_grad,
 *   out[c][2] the derivative with respect to noise[c];  info (classes, DEVICE int32): per class as pls_gp_mll_grad.
 * A non-positive pivot in class c is reported in info[c] alone: the call returns PLS_OK and the rows of the other classes
 * are valid.  The classes run one after another on `stream` and share the workspace of ONE evaluation:
 *   pls_gp_mll_classes_workspace_bytes_kind(kind, n, d, classes) = pls_gp_mll_workspace_bytes_kind(kind, n, d)   (16-byte
 *   aligned); pls_gp_mll_classes_workspace_bytes(n, d, classes) = pls_gp_mll_workspace_bytes(n, d). */
size_t pls_gp_mll_classes_workspace_bytes(int64_t n, int64_t d, int64_t classes);
size_t pls_gp_mll_classes_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d, int64_t classes);
int pls_gp_mll_grad_classes(int32_t kernel_kind, const double *x, int64_t n, int64_t d, int64_t classes,
                            const double *lengthscale /* device */, const double *outputscale /* host */,
                            const double *noise /* host */, const double *mean /* host */,
                            const double *fixed_noise /* device, may be NULL */, int64_t ldf, const double *y, int64_t ldy,
                            double jitter, double *out /* classes x (4 + d), RQ: (5 + d), PERIODIC: (4 + 2 d), LOCALLY_PERIODIC: (4 + 3 d) */, int32_t *info /* classes, device */,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Class probabilities of the Dirichlet GP at t test points from the latent means mu and variances var (classes x t,
 * leading dimensions ldmu, ldvar; device): the Monte-Carlo mean of the softmax under independent normals,
 *   out[i][c] = (1 / samples) sum_s softmax_c(mu[.][i] + sqrt(max(var[.][i], 0)) z[s][.])      out: t x classes (ldo), device
 * with z[s][c] element (row s, column c) of the library's normal matrix (PLS_NOISE_PHILOX) for step = first_point + i
 * under `seed`: the draws of a test point depend on its global index alone, so a batch of points can be split.
 * The softmax subtracts the maximum first.  Summation order: one wave per point; lane l adds the sample pairs
 * (s, s + 4), s = 8 (p / 4) + p % 4, of p = l, l + 64, ... in ascending order, then an xor butterfly over the 64 lanes
 * (offsets 32 ... 1), then the division by `samples`.  No atomics: two calls give the same bits.
 * classes <= 64; any samples >= 1 and t >= 1.  Nothing synchronises or allocates. */
int pls_softmax_normal_mean(const double *mu, int64_t ldmu, const double *var, int64_t ldvar, int64_t classes, int64_t t,
                            int64_t samples, uint64_t seed, uint64_t first_point, double *out, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse variational GP (SVGP) baseline: fixed kernel, fixed inducing points, Gaussian likelihood
 * ------------------------------------------------------------------------------------------- */

/* Replaces SVGP (src/gaussian_process/svgp.py:6-49), the minibatch loop of train_svgp with is_fixed=True
 * (experiments/trainers.py:55-136) and train_svgp_for_profiler (experiments/profiler/main.py:85-123).
 * RECALLED, not read: the arithmetic is gpytorch 1.15's whitened VariationalStrategy + CholeskyVariationalDistribution +
 * VariationalELBO + GaussianLikelihood as remembered (gpytorch is not available to this project); the formulas below are
 * the contract.
 *
 * Setup (the caller, from existing entries): K_zz = k(Z,Z) + jitter I = L L^T, A = L^-1 k(Z,X) (M x n), held transposed
 * as At (n x M, leading dimension ldat: one point's M values per row), q_i = k(x_i,x_i) + jitter - sum_p A_pi^2.
 * State (device): m (M), L_s (M x M, leading dimension ldls; ONLY the lower triangle and the diagonal are ever read or
 * written), scalars = {c, rho}: the constant mean and the raw noise, sigma^2 = softplus(rho) + 1e-4.
 * One minibatch idx[0 .. B), a_i row idx[i] of At:
 *   mu_i = c + a_i . m     w_i = L_s^T a_i     v_i = q_i + |w_i|^2
 *   l_i  = -1/2 log 2 pi - 1/2 log sigma^2 - ((y_i - mu_i)^2 + v_i) / (2 sigma^2)
 *   KL   = 1/2 (|tril L_s|_F^2 + |m|^2 - M - 2 sum_p log |L_s,pp|)          ELBO = (1/B) sum_i l_i - KL / n
 *   d/dm   = (1/B) sum_i g_mu,i a_i - m / n                                  g_mu,i = (y_i - mu_i) / sigma^2
 *   d/dL_s = tril[(2/B) sum_i g_v,i a_i w_i^T] - (tril L_s - diag(1 / L_s,pp)) / n      g_v,i = -1 / (2 sigma^2)
 *   d/dc   = (1/B) sum_i g_mu,i
 *   d/drho = sigmoid(rho) (1/B) sum_i [-1 / (2 sigma^2) + ((y_i - mu_i)^2 + v_i) / (2 sigma^4)]
 * Both contractions run on v_mfma_f64_16x16x4_f64; every sum has a fixed order (no atomics): two calls give the same
 * bits, and the outputs depend on the CONTENT of idx only (NULL = rows 0 .. B-1 in order = an explicit identity list).
 * An index outside 0 .. n-1 is not read: its point becomes NaN.  Nothing synchronises or allocates. */
typedef enum {
  PLS_SVGP_GAUSSIAN = 0,   /* the only one pls_svgp_elbo_grad / pls_svgp_sgd_epoch accept (closed-form epilogue) */
  PLS_SVGP_BERNOULLI = 1,  /* probit; through the pls_svgp_lik_* entries below */
  PLS_SVGP_STUDENT_T = 2   /* fixed degrees of freedom; through the pls_svgp_lik_* entries below */
} pls_svgp_likelihood;

typedef enum {
  PLS_SVGP_TRAIN_MEAN = 1,   /* pls_svgp_sgd_epoch updates c */
  PLS_SVGP_TRAIN_NOISE = 2   /* pls_svgp_sgd_epoch updates rho */
} pls_svgp_flags;

typedef struct {
  const double *At;   /* n x m, leading dimension ldat (columns m .. ldat-1 are never read) */
  int64_t ldat;
  const double *q;    /* n */
  const double *y;    /* n */
  int64_t n;
  int64_t m;          /* 1 .. 256 inducing points */
  int32_t likelihood; /* pls_svgp_likelihood */
  int32_t reserved;
} pls_svgp_desc;

/* Workspace of the calls below (8-byte aligned), with MP = m rounded up to 16 and T(k) = ceil(k / 32) tiles of 32 points:
 *   pls_svgp_workspace_bytes(n, m, batch) = 8 max(4 + 4 max(T(n), T(batch)),  4 + 4 T(batch) + T(batch) MP (MP + 1))
 * (3 KL sums; 3 scalar partials per tile; per tile of a gradient call MP partials of d/dm and an MP x MP partial of
 * d/dL_s).  pls_svgp_elbo_grad over b points needs the formula with n = batch = b at most. */
size_t pls_svgp_workspace_bytes(int64_t n, int64_t m, int64_t batch);

/* One evaluation.  idx: device int64, B entries, or NULL.  out (5, device or mapped pinned host): out[0] = ELBO,
 * out[1] = d/dc, out[2] = d/drho, out[3] = (1/B) sum l_i, out[4] = KL.  grad_m (M), grad_L (M x M, ldgl; only the lower
 * triangle is written): gradients of the ELBO.  grad_m == NULL && grad_L == NULL selects the value-only kernel, which
 * skips the second contraction; its out equals the full call's bit for bit.  Two launches. */
int pls_svgp_elbo_grad(const pls_svgp_desc *desc, const double *m, const double *L_s, int64_t ldls,
                       const double *scalars /* {c, rho}, device */, const int64_t *idx, int64_t b, double *out,
                       double *grad_m, double *grad_L, int64_t ldgl, void *workspace, size_t workspace_bytes, void *stream);

/* One epoch of plain SGD on loss = -ELBO (the inner loop of experiments/trainers.py:120-127): the ceil(n / batch_size)
 * minibatches perm[0 .. batch_size), perm[batch_size .. ), ... in order (perm: n device int64; the last batch is ragged and
 * divides by its own length), each followed by p <- p - lr * dloss/dp for m, tril L_s, and c / rho where `flags` has
 * PLS_SVGP_TRAIN_MEAN / PLS_SVGP_TRAIN_NOISE.  The update is a multiply followed by a subtract (no contraction), so a
 * replay through pls_svgp_elbo_grad gives the same bits.  Then loss_out[0] (device or mapped pinned host) = -ELBO of the
 * updated state over all n rows in order (the value-only evaluation).  Two launches per minibatch and two for the loss;
 * the host does not touch the state in between. */
int pls_svgp_sgd_epoch(const pls_svgp_desc *desc, double *m, double *L_s, int64_t ldls, double *scalars, const int64_t *perm,
                       int64_t batch_size, double lr, int32_t flags, double *loss_out, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Prediction at t points from their rows At_test (t x m, ldat) and q_test (t):  mean_out[i] = c + a_i . m,
 * var_out[i] = q_i + |L_s^T a_i|^2 (the latent variance; the observation variance adds sigma^2).  scalars as above
 * (device; only c is read).  One launch. */
int pls_svgp_predict(const double *m, const double *L_s, int64_t ldls, const double *scalars, const double *At_test,
                     int64_t ldat, const double *q_test, int64_t t, int64_t mdim, double *mean_out, double *var_out,
                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * SVGP with a quadrature likelihood (Bernoulli, Student-t)
 * ------------------------------------------------------------------------------------------- */

/* Replaces SVGP(..., likelihood=BernoulliLikelihood()) of the two classification drivers
 * (experiments/curves/classification/main.py:324-361, experiments/uci/classification/main.py:267-277) and the
 * `svgp-student` model of experiments/uci/regression/main.py:353-401 (StudentTLikelihood, degrees of freedom pinned).
 * RECALLED, not read: gpytorch 1.15's BernoulliLikelihood, StudentTLikelihood and the Gauss-Hermite quadrature of
 * _OneDimensionalLikelihood.expected_log_prob (20 nodes by default) as remembered; gpytorch is not available to this
 * project and the formulas below are the contract.
 *
 * mu_i, w_i, v_i, KL, the ELBO and the assembly d/dm, d/dL_s, d/dc are those of the SVGP section above; only the per-point
 * terms l_i, g_mu,i, g_v,i differ.  With Q = 20, x_k and omega_k the nodes and weights of
 * numpy.polynomial.hermite.hermgauss(20) as doubles (17 significant digits in csrc/svgp.hip) and w^_k = omega_k / sqrt(pi)
 * rounded once:
 *   f_k = mu_i + sqrt(2 v_i) x_k        l_i = sum_k w^_k g(f_k)
 *   g_mu,i = sum_k w^_k g'(f_k)         g_v,i = (sum_k w^_k g'(f_k) x_k) / sqrt(2 v_i)
 * the derivatives of the quadrature SUM (what autograd on gpytorch yields), not quadratures of derivatives.  They need
 * v_i > 0: a point with v_i <= 0 becomes non-finite and shows in every output, as an out-of-range index does.
 *
 * PLS_SVGP_BERNOULLI (probit): y in {0, 1}, s = 2 y - 1, g(f) = log Phi(s f), g'(f) = s phi(s f) / Phi(s f), accurate in
 * the tails: for z < 0  log Phi(z) = log(erfcx(-z / sqrt 2) / 2) - z^2 / 2 and phi / Phi = sqrt(2 / pi) / erfcx(-z / sqrt 2);
 * for z >= 0  log Phi(z) = log1p(-erfc(z / sqrt 2) / 2).  No likelihood parameter: out[2] = 0 exactly and rho is never
 * written, PLS_SVGP_TRAIN_NOISE or not.  Prediction: obs_out = p (1 - p) at p = Phi(mu / sqrt(1 + v)).
 *
 * PLS_SVGP_STUDENT_T: scale^2 = s^2 = noise = softplus(rho) (gpytorch's Positive constraint: NO 1e-4 floor, unlike the
 * Gaussian likelihood's softplus(rho) + 1e-4).  nu = deg_free is a constant: the reference pins it inside an interval of
 * width 2e-10, so its raw value's gradient is of order 1e-10 and is taken as 0.  With r = y - f:
 *   g      = lgamma((nu + 1) / 2) - lgamma(nu / 2) - 1/2 log(nu pi s^2) - (nu + 1) / 2 log1p(r^2 / (nu s^2))
 *   g'     = (nu + 1) r / (nu s^2 + r^2)
 *   dg/ds2 = -1 / (2 s^2) + (nu + 1) r^2 / (2 s^2 (nu s^2 + r^2))
 *   d/drho = sigmoid(rho) (1/B) sum_i sum_k w^_k dg/ds2(f_k)
 * Prediction: obs_out = v + s^2 nu / (nu - 2).
 *
 * PLS_SVGP_GAUSSIAN through these entries: the bits of pls_svgp_elbo_grad / pls_svgp_sgd_epoch / pls_svgp_predict, and
 * obs_out = v + sigma^2.
 *
 * The workspace is pls_svgp_workspace_bytes; the launches, the order of every sum and the promises of the SVGP section
 * (two calls the same bits, the value-only call equals the full call, the outputs depend on the content of idx only) are
 * the same.  Per point the nodes are added in a fixed order: 8 lanes, lane s adds nodes s, s + 8, s + 16, then an xor
 * butterfly.  Validation comes before any HIP call: an unknown likelihood, a Student-t deg_free that is not finite or
 * not > 2, and everything the SVGP entries check. */
typedef struct {
  pls_svgp_desc base; /* base.likelihood: any pls_svgp_likelihood */
  double deg_free;    /* Student-t: nu > 2, fixed; ignored otherwise */
} pls_svgp_lik_desc;

/* pls_svgp_elbo_grad with the descriptor's likelihood (out[2] = d/drho: 0 for Bernoulli). */
int pls_svgp_lik_elbo_grad(const pls_svgp_lik_desc *desc, const double *m, const double *L_s, int64_t ldls,
                           const double *scalars /* {c, rho}, device */, const int64_t *idx, int64_t b, double *out,
                           double *grad_m, double *grad_L, int64_t ldgl, void *workspace, size_t workspace_bytes,
                           void *stream);

/* pls_svgp_sgd_epoch with the descriptor's likelihood; a replay through pls_svgp_lik_elbo_grad gives the same bits. */
int pls_svgp_lik_sgd_epoch(const pls_svgp_lik_desc *desc, double *m, double *L_s, int64_t ldls, double *scalars,
                           const int64_t *perm, int64_t batch_size, double lr, int32_t flags, double *loss_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* pls_svgp_predict (the same bits in mean_out and var_out) and, where obs_out != NULL, the variance of an observation
 * under the likelihood as stated above (t doubles).  Of desc only base.likelihood and deg_free are read; scalars: c and,
 * for the Gaussian and Student-t likelihoods, rho.  One launch. */
int pls_svgp_lik_predict(const pls_svgp_lik_desc *desc, const double *m, const double *L_s, int64_t ldls,
                         const double *scalars, const double *At_test, int64_t ldat, const double *q_test, int64_t t,
                         int64_t mdim, double *mean_out, double *var_out, double *obs_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Symmetric eigendecomposition (csrc/sym_eigh.hip: two-sided cyclic Jacobi, blocked, fp64 MFMA)
 * ------------------------------------------------------------------------------------------- */

/* A = V diag(lam) V^T for the symmetric m x m matrix whose LOWER triangle A holds (row-major, pitch lda; the strict upper
 * triangle is never read, as torch.linalg.eigh reads by default; A is not written).  Replaces `torch.linalg.eigh` at
 * orthonormal.py:46-48 (k(Z,Z) / M of the orthonormal basis) and samplers.py:27 (the indefinite predictive covariance).
 * lam: m doubles, ascending.  V (m x m, pitch ldv): column k is the eigenvector of lam[k]; its largest-magnitude
 * component (the first one on ties) is positive, so the result has ONE gauge: the same bits on every call of a build.
 * info (HOST memory): 0 = converged; 1 = the sweep cap (30) was reached -- lam and V are the last iterate, and the call
 * still returns PLS_OK.
 * m <= 64: one workgroup diagonalises the matrix in LDS.  m > 64: blocks of 32, a round-robin over block pairs, three
 * launches per round.  A pair (p, q) rotates only while |s_pq| > eps ||A||_F / m.
 * m == 0 returns PLS_OK and touches nothing.  NULL pointers, lda < m, ldv < m, m < 0 and a workspace shorter than
 * pls_sym_eigh_workspace_bytes(m) return PLS_ERR_INVALID_ARGUMENT before any HIP call; a NaN or an infinity in the lower
 * triangle returns PLS_ERR_INVALID_ARGUMENT ("non-finite") after the first reduction, without sweeping.
 * SYNCHRONISES `stream`: once after that reduction and once per outer sweep (the host reads the sweep's rotation count
 * from pinned memory).  The call can therefore not be captured in a graph.  It allocates 64 pinned bytes on a thread's
 * first call and nothing afterwards.  workspace: device memory, 8-byte aligned. */
size_t pls_sym_eigh_workspace_bytes(int64_t m);
int pls_sym_eigh(const double *A, int64_t lda, int64_t m, double *lam, double *V, int64_t ldv, int32_t *info,
                 void *workspace, size_t workspace_bytes, void *stream);
/* The block pairs (I < J) of one round of the solver's schedule for nblocks >= 2 blocks, round in [0, nblocks - 1) for an
 * even and [0, nblocks) for an odd count: pairs[2 k], pairs[2 k + 1] for k < the returned count (room for nblocks / 2
 * pairs).  The pairs of a round are disjoint; every unordered pair occurs once per sweep; with an odd count one block per
 * round has a bye.  Pure host code; 0 for arguments outside those ranges. */
int64_t pls_sym_eigh_round_pairs(int64_t nblocks, int64_t round, int64_t *pairs);

/* ---------------------------------------------------------------------------------------------
 * Orthonormal basis: setup + step
 * ------------------------------------------------------------------------------------------- */

/* A = Vs^T Kzx and At = Kzx^T Vs from the scaled eigenvectors Vs (M x Mk) and Kzx (M x N).
 * Replaces the per-step re-association `base_gram_induce_train.T @ scaled_eigenvectors`
 * (orthonormal.py:106-108) and `scaled_eigenvectors.T @ base_gram_induce_train` (:152-154) by a one-time build. */
int pls_onb_build_projection(const double *Vs, int64_t ldvs, const double *Kzx, int64_t ldkzx, int64_t m, int64_t mk,
                             int64_t n, double *A, int64_t lda, double *At, int64_t ldat, void *stream);

/* Gaussian/identity fast path constants: B = A A^T (Mk x Mk), c[0..Mk) = A y and c[Mk] = y^T y (c holds Mk + 1 doubles). */
int pls_onb_build_gaussian(const pls_onb_desc *basis, const double *y, double *B, int64_t ldb, double *c,
                           void *stream);

/* F(N x J) = A^T U.  Replaces OrthonormalBasis.calculate_untransformed_train_prediction_samples
 * (orthonormal.py:98-108).  Leading dimensions: lda, ldu as contraction operands, ldf as a contraction output (see
 * "Leading dimensions" above). */
int pls_onb_forward(const pls_onb_desc *basis, const double *U, int64_t ldu, int64_t j, double *F, int64_t ldf,
                    void *stream);

/* dU(Mk x J) = -eta * A G - eta * diag(1/lam) U + sqrt(2 eta) * xi.
 * Replaces OrthonormalBasis._calculate_particle_update (orthonormal.py:128-159).
 * Leading dimensions: ldat, ldg as contraction operands; ldu, lddu any. */
int pls_onb_particle_update(const pls_onb_desc *basis, const double *U, int64_t ldu, const double *G, int64_t ldg,
                            int64_t j, double eta, const pls_noise_desc *noise, double *dU, int64_t lddu,
                            void *stream);

/* One fused Langevin step: PLS.calculate_particle_update(U, eta)
 * (projected_langevin_sampling.py:107-123 -> orthonormal.py:98-108 -> costs/{*}.py -> orthonormal.py:128-159).
 * Streams N in chunks: F chunk -> cost derivative in the GEMM epilogue -> back-projection; F and G are
 * never materialised beyond one chunk.  If basis->B/c are set and the cost is Gaussian/identity the
 * Mk x Mk x J fast path is taken unless force_generic != 0.
 * out_mode 0: out = dU (the reference's return value);  out_mode 1: out = U + dU (the caller's
 * `particles += update`, trainers.py:157, fused).  out must not alias U: other workgroups still read U as
 * the GEMM operand, so callers ping-pong two particle buffers.
 * energy_in (may be NULL): receives e_j(U) of the INPUT particles -- the value pls_onb_energy returns -- as a
 * by-product: on the fast path from the same B U product (2 * cdiv(mk, 128) * j workspace doubles hold every tiling; a launch of
 * 64-row tiles leaves cdiv(mk, 64) partial rows and takes a workspace of that many, never fewer), otherwise
 * from the same F tile the cost derivative is taken of, so a train loop (trainers.py:153-159, which recomputes F for the
 * energy) pays no separate energy pass.
 * workspace: pls_onb_step_workspace_bytes(...) bytes (any larger size lets it use bigger N chunks).  The query covers every
 * route the call may take: for a basis of at most 128 functions it is the larger of the general route's layout for chunks of
 * n_chunk rows and the one-launch step's (its row slabs, and its counters where the caller brings none).  A smaller workspace
 * is not refused while it holds the layout of a route that applies -- the one-launch step first, else the general route in
 * chunks of at least min(n, 128) rows -- and PLS_ERR_WORKSPACE_TOO_SMALL means that it holds neither.
 * Leading dimensions (this and every other pls_onb_* / pls_ipb_* step, update and energy entry): the descriptor's matrices and
 * the particles are contraction operands; ldo, ldxi any; the fused small-rank kernels and the solve-and-noise launch are routed
 * around their limits; the solves follow pls_chol_solve (see "Leading dimensions" above). */
size_t pls_onb_step_workspace_bytes(const pls_onb_desc *basis, int64_t j, int64_t n_chunk);
int pls_onb_step(const pls_onb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu,
                 int64_t j, double eta, const pls_noise_desc *noise, double *out, int64_t ldo, int32_t out_mode,
                 int32_t force_generic, double *energy_in, void *workspace, size_t workspace_bytes, void *stream);

/* out[b] = the sum of e[16 b .. min(j, 16 (b + 1))) in ascending order (pls_block_desc.energy_sums16 as a stand-alone launch). */
int pls_sums16(const double *e, int64_t j, double *out, void *stream);
/* Number of 32-bit counters behind pls_block_desc.step_sync for j particle columns. */
size_t pls_step_sync_words(int64_t j);
/* Bytes of pls_block_desc.energy_partials for a basis with `rows` functions (Mk, or M of the inducing-point basis) and j
 * particle columns. */
size_t pls_energy_partials_bytes(int64_t rows, int64_t j);

/* The Winograd route of the general step (ABI 6; csrc/winograd.h, PLS_OPT_WINOGRAD).  pls_onb_winograd_bytes: bytes of the
 * basis' left-hand planes S1..S4 (N/2 x M_k/2 doubles each, 256-byte aligned), 0 where the route does not apply: M_k a
 * multiple of 16 and >= 512, N a multiple of 4 and >= 16384, A / At 16-byte aligned with even leading dimensions.
 * pls_onb_winograd_prepare builds them from At (once per basis; again only if At changes) into `planes` (16-byte aligned).
 * pls_onb_step_wg / pls_onb_step_blocks_wg are pls_onb_step / pls_onb_step_blocks with the planes (wg_planes, wg_bytes)
 * handed in; wg_planes NULL: exactly pls_onb_step / pls_onb_step_blocks.  The route pairs data row n with n + N/2 and particle
 * column j with j + J/2, so a J-shard and the whole particle matrix agree to rounding, not bit for bit.  Its workspace is
 * no larger than the plain route's: it is taken where the workspace handed in (pls_onb_step_workspace_bytes) holds its
 * chunks, else the plain route runs. */
size_t pls_onb_winograd_bytes(const pls_onb_desc *basis);
int pls_onb_winograd_prepare(const pls_onb_desc *basis, double *planes, size_t planes_bytes, void *stream);
int pls_onb_step_wg(const pls_onb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu, int64_t j,
                    double eta, const pls_noise_desc *noise, double *out, int64_t ldo, int32_t out_mode, int32_t force_generic,
                    const double *wg_planes, size_t wg_bytes, double *energy_in, void *workspace, size_t workspace_bytes,
                    void *stream);
int pls_onb_step_blocks_wg(const pls_onb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu,
                           int64_t j, const pls_block_desc *blocks, const pls_noise_desc *noise, double *out, int64_t ldo,
                           int32_t out_mode, int32_t force_generic, const double *wg_planes, size_t wg_bytes, double *energy_in,
                           void *workspace, size_t workspace_bytes, void *stream);

/* pls_onb_step with one step size PER COLUMN BLOCK (pls_block_desc): the batched step-size search. */
int pls_onb_step_blocks(const pls_onb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu,
                        int64_t j, const pls_block_desc *blocks, const pls_noise_desc *noise, double *out, int64_t ldo,
                        int32_t out_mode, int32_t force_generic, double *energy_in, void *workspace,
                        size_t workspace_bytes, void *stream);

/* e(J) = cost_j + 0.5 * sum_m U_mj^2 / lam_m  (per-particle energy; the caller takes the mean over all
 * particles of all ranks).  Replaces PLS.calculate_energy_potential -> OrthonormalBasis.calculate_energy_potential
 * (projected_langevin_sampling.py:125-138, orthonormal.py:110-126).
 * Gaussian/identity with basis->B/c set (and force_generic == 0): cost_j = (u_j^T B u_j - 2 c^T u_j + y^T y) / (2 sigma2)
 * from ONE Mk x Mk x J contraction instead of the N x Mk x J one.
 * Leading dimensions: ldu, lda, ldat, ldb as contraction operands; ldat beyond 2^23 is ROUTED from the fused small-rank
 * kernel to the contractions (above). */
size_t pls_onb_energy_workspace_bytes(const pls_onb_desc *basis, int64_t j, int64_t n_chunk);
int pls_onb_energy(const pls_onb_desc *basis, const pls_cost_desc *cost, const double *y, const double *U,
                   int64_t ldu, int64_t j, double *e, int32_t force_generic, void *workspace, size_t workspace_bytes,
                   void *stream);

/* e(J) = cost_j + 0.5 * sum_m U_mj^2 / lam_m with the cost vector handed in (cost may be NULL = zeros).
 * Replaces OrthonormalBasis.calculate_energy_potential(particles, cost) (orthonormal.py:110-126) before its
 * .mean().item(). */
int pls_onb_prior_energy(const pls_onb_desc *basis, const double *U, int64_t ldu, int64_t j, const double *cost,
                         double *e, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Inducing-point basis: step (setup = pls_kernel_gram + pls_chol_factor)
 * ------------------------------------------------------------------------------------------- */

/* F = Kxz k(Z,Z)^-1 U (inducing_point.py:81-93). workspace: m*j doubles.
 * Leading dimensions: ldu as the solve's right-hand side (a contraction operand with the inverse factor, the substitution
 * kernel's limit without it), ldkzx as a contraction operand, ldf as a contraction output (above). */
int pls_ipb_forward(const pls_ipb_desc *basis, const double *U, int64_t ldu, int64_t j, double *F, int64_t ldf,
                    void *workspace, size_t workspace_bytes, void *stream);

/* dU = -eta Kzx G - eta M k(Z,Z)^-1 U + sqrt(2 eta) e, e = Lc xi (inducing_point.py:117-150).
 * PLS_NOISE_INJECTED: noise->xi is used AS e (already coloured).
 * workspace: 4 * align256(m*j*8) bytes. */
int pls_ipb_particle_update(const pls_ipb_desc *basis, const double *U, int64_t ldu, const double *G, int64_t ldg,
                            int64_t j, double eta, const pls_noise_desc *noise, double *dU, int64_t lddu,
                            void *workspace, size_t workspace_bytes, void *stream);

size_t pls_ipb_step_workspace_bytes(const pls_ipb_desc *basis, int64_t j, int64_t n_chunk);
/* energy_in (optional, J doubles): receives the energy of the INPUT particles (cost of the same F the drift uses +
 * the prior term) as a by-product, like pls_onb_step.  If basis->B/c are set and the cost is Gaussian/identity the
 * M x M x J fast path is taken unless force_generic != 0.  Other costs on at most 128 inducing points take, while the
 * problem is launch-bound (PLS_OPT_SMALL_RANK_STEP), two launches: V = k(Z,Z)^-1 U with the coloured noise (csrc/ipb_prep.h,
 * PLS_OPT_IPB_PREP), then projection, cost, back-projection, prior drift, update and energies in one
 * (csrc/small_rank_step.h; pls_block_desc.step_sync / energy_sums16 apply as for pls_onb_step_blocks). */
int pls_ipb_step(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu,
                 int64_t j, double eta, const pls_noise_desc *noise, double *out, int64_t ldo, int32_t out_mode,
                 int32_t force_generic, double *energy_in, void *workspace, size_t workspace_bytes, void *stream);

/* 1 if the two-launch route of pls_ipb_step would solve and colour the noise in the launch of csrc/ipb_prep.h for this
 * descriptor under the calling thread's options (philox != 0: Philox noise, which LcT colours), 0 if it takes the separate
 * solve and noise launches; the step's own predicate, nothing is launched.  Leading dimensions: 0 when ldlinv, ldlinvt
 * (or, with philox, ldlct) exceeds pls_ld_limit(PLS_LD_IPB_PREP, m, 1). */
int pls_ipb_prep_applies(const pls_ipb_desc *basis, int32_t philox);

/* pls_ipb_step with one step size PER COLUMN BLOCK (pls_block_desc): the batched step-size search. */
int pls_ipb_step_blocks(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *y, double *U, int64_t ldu,
                        int64_t j, const pls_block_desc *blocks, const pls_noise_desc *noise, double *out, int64_t ldo,
                        int32_t out_mode, int32_t force_generic, double *energy_in, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Gaussian/identity fast path constants of the inducing-point basis: B = Kzx Kxz (M x M), c[0..M) = Kzx y, c[M] = y^T y.
 * With V = K^-1 U the data drift Kzx (Kxz V - y) / sigma2 (inducing_point.py:117-150 with gaussian.py:86-88) is
 * (B V - c) / sigma2 and the cost (gaussian.py:63-73) the quadratic form (v^T B v - 2 c^T v + y^T y) / (2 sigma2). */
int pls_ipb_build_gaussian(const pls_ipb_desc *basis, const double *y, double *B, int64_t ldb, double *c, void *stream);

/* e(J) = cost_j + (M/2) * ||k(Z,Z)^-1 U_j||^2 (inducing_point.py:95-115). */
size_t pls_ipb_energy_workspace_bytes(const pls_ipb_desc *basis, int64_t j, int64_t n_chunk);
int pls_ipb_energy(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *y, const double *U,
                   int64_t ldu, int64_t j, double *e, int32_t force_generic, void *workspace, size_t workspace_bytes, void *stream);

/* Whitened coordinates S = Lc^-1 U of the inducing-point basis, Gaussian cost with the identity link.
 * With V = k(Z,Z)^-1 U = Lc^-T S the update of inducing_point.py:117-150 under gaussian.py:86-88,
 *     dU = -eta ((B V - c) / sigma2 + M V) + sqrt(2 eta) Lc xi,
 * is  dU = Lc dS,  dS = -eta (Q S - ct) + sqrt(2 eta) xi,  and the energy of inducing_point.py:95-115 is
 * S^T Q S / 2 - ct^T S + y^T y / (2 sigma2): the same law, the same noise xi, one M x M x J contraction per step.
 * pls_ipb_build_whitened: Q (M x M, 16-byte aligned, ldq even) and ct (M + 1 doubles) from the descriptor's B, c and
 * Cholesky operators for inv_noise = 1 / sigma2; the caller then stores Q, ldq, ct and q_inv_noise = inv_noise in the
 * descriptor.  workspace: pls_ipb_build_whitened_workspace_bytes(M). */
size_t pls_ipb_build_whitened_workspace_bytes(int64_t m);
int pls_ipb_build_whitened(const pls_ipb_desc *basis, double inv_noise, double *Q, int64_t ldq, double *ct, void *workspace,
                           size_t workspace_bytes, void *stream);
/* Pt (M x M, 16-byte aligned, ldpt even) = Lc^-T Q from the descriptor's Linv and Q (see pls_ipb_desc.Pt); rebuilt whenever
 * Q is. */
int pls_ipb_build_step_operator(const pls_ipb_desc *basis, double *Pt, int64_t ldpt, void *stream);
/* S = Lc^-1 U and back, U = Lc S (neither may alias its input). */
int pls_ipb_whiten(const pls_ipb_desc *basis, const double *U, int64_t ldu, int64_t j, double *S, int64_t lds, void *stream);
int pls_ipb_unwhiten(const pls_ipb_desc *basis, const double *S, int64_t lds, int64_t j, double *U, int64_t ldu, void *stream);
/* One Langevin step of the whitened particles: out = dS (out_mode 0) or S + dS (out_mode 1); Philox noise draws the xi
 * of the reference's e = Lc xi (same counters as pls_ipb_step), injected noise is used as xi (NOT coloured).  energy_in
 * (optional): energy of the INPUT particles; pls_ipb_whitened_workspace_bytes(basis, J) = 2 cdiv(M, 128) J doubles hold its
 * partial rows under every tiling (a launch of 64-row tiles takes cdiv(M, 64) J doubles, as pls_onb_step's fast path). */
size_t pls_ipb_whitened_workspace_bytes(const pls_ipb_desc *basis, int64_t j);
int pls_ipb_whitened_step(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *S, int64_t lds, int64_t j,
                          double eta, const pls_noise_desc *noise, double *out, int64_t ldo, int32_t out_mode, double *energy_in,
                          void *workspace, size_t workspace_bytes, void *stream);
/* The same for ANY cost, on at most 128 inducing points, in ONE launch (csrc/small_rank_step.h over pls_ipb_desc.Awa): dS =
 * -eta Awa^T g + sqrt(2 eta) xi with g = d cost / d f on the data rows and f on the prior rows -- inducing_point.py:117-150 in
 * whitened coordinates, no solve and no coloured noise per step (a training loop whitens once, unwhitens once).  y: the n targets.
 * blocks: step sizes, and step_sync / energy_sums / energy_sums16 as for pls_onb_step_blocks.  _applies: 1 if the descriptor,
 * the targets' alignment and the sizes allow it (else the caller stays in the original coordinates: pls_ipb_step). */
int pls_ipb_build_whitened_operand(const pls_ipb_desc *basis, double *Awa, int64_t ldawa, void *stream);
int pls_ipb_whitened_generic_applies(const pls_ipb_desc *basis, const double *y, int64_t j);
size_t pls_ipb_whitened_generic_workspace_bytes(const pls_ipb_desc *basis, int64_t j);
int pls_ipb_whitened_generic_step(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *y, const double *S,
                                  int64_t lds, int64_t j, double eta, const pls_block_desc *blocks, const pls_noise_desc *noise,
                                  double *out, int64_t ldo, int32_t out_mode, double *energy_in, void *workspace,
                                  size_t workspace_bytes, void *stream);
int pls_ipb_whitened_step_blocks(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *S, int64_t lds, int64_t j,
                                 const pls_block_desc *blocks, const pls_noise_desc *noise, double *out, int64_t ldo,
                                 int32_t out_mode, double *energy_in, void *workspace, size_t workspace_bytes, void *stream);
/* e(J) of whitened particles; workspace: pls_ipb_whitened_workspace_bytes(basis, J). */
int pls_ipb_whitened_energy(const pls_ipb_desc *basis, const pls_cost_desc *cost, const double *S, int64_t lds, int64_t j,
                            double *e, void *workspace, size_t workspace_bytes, void *stream);

/* e(J) = cost_j + (M/2) * ||k(Z,Z)^-1 U_j||^2 with the cost vector handed in (inducing_point.py:95-115).
 * workspace: m*j doubles. */
int pls_ipb_prior_energy(const pls_ipb_desc *basis, const double *U, int64_t ldu, int64_t j, const double *cost,
                         double *e, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Setup before the path: greedy conditional-variance inducing-point selection
 * ------------------------------------------------------------------------------------------- */

/* Picks m rows of x (N x D, row-major) by the partial pivoted Cholesky / greedy DPP-MAP rule of
 * src/inducing_point_selectors/conditional_variance.py:27-120 (the caller has already applied the reference's random
 * permutation, :58-61): start from argmax of the jittered kernel diagonal, then repeatedly
 *   e = (round20(k(X, x_j)) + jitter * [n == j] - c[:i, j] . c[:i, :]) / sqrt(d_j);  c[i, :] = e;  d = max(d - e^2, 0)
 * and take the largest remaining d among the points not chosen yet (:101-106); stop early once sum(d) < threshold
 * (:108-113).  No N x N Gram matrix is formed (the reference builds one just to read its diagonal, :64-69).
 * indices: m int64 (device), count: 1 int64 (device) = number of points selected (m unless the threshold stopped it).
 * Nothing synchronises: the pivot of every iteration stays on the device.  Ties are broken towards the smaller index.
 * kernel_kind: any pls_kernel_kind; lengthscale: d values (every kind except LINEAR needs it; ignored for LINEAR; RQ: d + 1; PERIODIC: 2 d, d <= 16; LOCALLY_PERIODIC: 3 d, d <= 16; TREND_SEASONAL: 4 d + 1, d <= 8).
 * workspace: pls_select_inducing_workspace_bytes(n, m) bytes. */
size_t pls_select_inducing_workspace_bytes(int64_t n, int64_t m);
int pls_select_inducing_conditional_variance(int32_t kernel_kind, const double *x, int64_t n, int64_t d,
                                             const double *lengthscale, double outputscale, int64_t m, double jitter,
                                             double threshold, int64_t *indices, int64_t *count, void *workspace,
                                             size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PLSHIP_H */
