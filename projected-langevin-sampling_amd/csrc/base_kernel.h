// What the pairwise kernels of base_kernel.hip share (Gram build, gradient reduction, fused predictive mean): tile geometry,
// the pre-scaled staging of the points, the distance sum of a pair, the KIND x D_MAX dispatch.  The pair's value: kernel_math.h.
// The periodic kind is not a function of one distance sum: its points are staged UNSCALED, its two scales per coordinate
// sit in LDS, and its pair loop (periodic_exponent, periodic_factors) evaluates every coordinate on its own.  The locally
// periodic kind does the same with a third scale per coordinate, the envelope's 1 / l_k (locally_periodic_exponent,
// locally_periodic_factors).  The trend-plus-seasonal kind is the locally periodic one with a fourth scale per coordinate, the
// trend's 1 / l_k, and a second sum beside the exponent (trend_seasonal_exponents, trend_seasonal_factors).
#pragma once
#include "common.h"
#include "kernel_math.h"

namespace plship {

// A workgroup of the Gram build or of the reduction covers PAIR_ROWS rows x PAIR_COLS columns of the pair matrix: 256
// threads, a pair of columns each, walking down the rows.  PAIR_D_MAX: the largest input dimension of every pairwise kernel.
constexpr int PAIR_ROWS = 64, PAIR_COLS = 512, PAIR_D_MAX = 64;
// the periodic kind's own limit: its reduction carries 2 D_MAX + 1 accumulators per thread, at 16 what RBF carries at 32
constexpr int PERIODIC_D_MAX = 16;
// the kinds whose points are staged unscaled and whose coordinates go through periodic_coord; the first two share
// PERIODIC_D_MAX (the locally periodic reduction carries 3 D_MAX + 1 accumulators and splits a column's coordinates in two
// halves above 8)
constexpr bool periodic_like(int kind) {
  return kind == PLS_KERNEL_PERIODIC || kind == PLS_KERNEL_LOCALLY_PERIODIC || kind == PLS_KERNEL_TREND_SEASONAL;
}
// the trend-plus-seasonal kind's own limit: its reduction carries 4 D_MAX + 2 accumulators per thread, 34 at 8 (the locally
// periodic kind carries 49 at 16); at 16 they would be 66 beside the factors
constexpr int TREND_SEASONAL_D_MAX = 8;
static inline int64_t kind_d_max(int32_t kind) {
  return kind == PLS_KERNEL_TREND_SEASONAL ? TREND_SEASONAL_D_MAX : periodic_like(kind) ? PERIODIC_D_MAX : PAIR_D_MAX;
}

// pls_kernel_mean: test points of a workgroup (one per lane, the four waves split the training points), and the training
// points staged in LDS at a time: 32 KiB of pre-scaled coordinates, 512 points at the most; a multiple of 4 for every D_MAX
constexpr int MEAN_POINTS = 64;
constexpr int mean_chunk(int d_max) { return 4096 / d_max < 512 ? 4096 / d_max : 512; }

// shape parameters of a kind: they follow the d lengthscales in its `lengthscale` argument (RQ: alpha; periodic: the d
// period lengths; locally periodic: the d periodic lengthscales, then the d period lengths; trend plus seasonal: the seasonal
// term's d envelope lengthscales, d periodic lengthscales and d period lengths, then its outputscale)
static inline int64_t kind_shape_params(int32_t kind, int64_t d) {
  return kind == PLS_KERNEL_RQ ? 1 : kind == PLS_KERNEL_PERIODIC ? d : kind == PLS_KERNEL_LOCALLY_PERIODIC ? 2 * d :
         kind == PLS_KERNEL_TREND_SEASONAL ? 3 * d + 1 : 0;
}
// sums of the reduction: the kappa sum, one per lengthscale, one per shape parameter
static inline int64_t grad_sums_count(int32_t kind, int64_t d) { return d + 1 + kind_shape_params(kind, d); }

// workgroups of the reduction over an n x n matrix = partial rows of grad_sums_count doubles in its workspace
static inline int64_t grad_sums_blocks(int64_t n) { return cdiv(n, PAIR_COLS) * cdiv(n, PAIR_ROWS); }
static inline size_t grad_sums_workspace_bytes(int32_t kind, int64_t n, int64_t d) {
  return (size_t)grad_sums_blocks(n) * (size_t)grad_sums_count(kind, d) * sizeof(double);
}

static inline bool stationary_kind(int32_t kind) {
  return kind == PLS_KERNEL_RBF_ARD || kind == PLS_KERNEL_MATERN12 || kind == PLS_KERNEL_MATERN32 || kind == PLS_KERNEL_MATERN52 ||
         kind == PLS_KERNEL_RQ || periodic_like(kind);
}
// what every entry checks after the kind and d >= 1: the kind's largest input dimension, under the entry's name `who`
static inline int check_kind_dim(const char *who, int32_t kind, int64_t d) {
  PLS_REQUIRE(kind != PLS_KERNEL_PERIODIC || d <= PERIODIC_D_MAX,
              "%s: input dimension %lld > 16 is not supported for the periodic kernel", who, (long long)d);
  PLS_REQUIRE(kind != PLS_KERNEL_LOCALLY_PERIODIC || d <= PERIODIC_D_MAX,
              "%s: input dimension %lld > 16 is not supported for the locally periodic kernel", who, (long long)d);
  PLS_REQUIRE(kind != PLS_KERNEL_TREND_SEASONAL || d <= TREND_SEASONAL_D_MAX,
              "%s: input dimension %lld > 8 is not supported for the trend-plus-seasonal kernel", who, (long long)d);
  PLS_REQUIRE(d <= PAIR_D_MAX, "%s: input dimension %lld > 64 is not supported", who, (long long)d);
  return PLS_OK;
}

// What pls_kernel_grad_sums, pls_gp_mll_grad and pls_gp_mll_grad_classes check alike, each under its own name `who`: the
// kernel kind, the sizes (classes == NULL: the entry has no class axis), the grid limit of the reduction and the
// workspace of `need` bytes on an `align`-byte boundary.  The entry's own checks follow it.
int gp_check_shared(const char *who, int32_t kernel_kind, int64_t n, int64_t d, const int64_t *classes, const void *workspace,
                    size_t workspace_bytes, size_t need, int align);

// the reduction and its finishing launch (arguments already validated)
int grad_sums_launch(int kind, const double *x, int64_t n, int d, const double *lengthscale, double outputscale,
                     const double *alpha, const double *P, int64_t ldp, double *out, double *partials, hipStream_t st);

// The KIND x D_MAX instantiations of a base kernel's per-pair loops: f(integral_constant<KIND>, integral_constant<D_MAX>), D_MAX
// the input dimension rounded up to 1, 2, 4, ..., 64 (periodic and locally periodic: ..., 16; trend plus seasonal: ..., 8; kind
// and d already validated).  LINEAR: with the linear
// kind (the Gram build).
template <bool LINEAR, class F>
static int for_kind_dmax(int kind, int d, F &&f) {
  using std::integral_constant;
  auto with_kind = [&](auto k) {
    if (d <= 1) return f(k, integral_constant<int, 1>{});
    if (d <= 2) return f(k, integral_constant<int, 2>{});
    if (d <= 4) return f(k, integral_constant<int, 4>{});
    if (d <= 8) return f(k, integral_constant<int, 8>{});
    if (d <= 16) return f(k, integral_constant<int, 16>{});
    if (d <= 32) return f(k, integral_constant<int, 32>{});
    return f(k, integral_constant<int, 64>{});
  };
  if constexpr (LINEAR) if (kind == PLS_KERNEL_LINEAR) return with_kind(integral_constant<int, PLS_KERNEL_LINEAR>{});
  auto with_periodic_kind = [&](auto k) {
    if (d <= 1) return f(k, integral_constant<int, 1>{});
    if (d <= 2) return f(k, integral_constant<int, 2>{});
    if (d <= 4) return f(k, integral_constant<int, 4>{});
    if (d <= 8) return f(k, integral_constant<int, 8>{});
    return f(k, integral_constant<int, PERIODIC_D_MAX>{});
  };
  if (kind == PLS_KERNEL_PERIODIC) return with_periodic_kind(integral_constant<int, PLS_KERNEL_PERIODIC>{});
  if (kind == PLS_KERNEL_LOCALLY_PERIODIC) return with_periodic_kind(integral_constant<int, PLS_KERNEL_LOCALLY_PERIODIC>{});
  if (kind == PLS_KERNEL_TREND_SEASONAL) {
    const integral_constant<int, PLS_KERNEL_TREND_SEASONAL> k{};
    if (d <= 1) return f(k, integral_constant<int, 1>{});
    if (d <= 2) return f(k, integral_constant<int, 2>{});
    if (d <= 4) return f(k, integral_constant<int, 4>{});
    return f(k, integral_constant<int, TREND_SEASONAL_D_MAX>{});
  }
  switch (kind) {
    case PLS_KERNEL_RBF_ARD: return with_kind(integral_constant<int, PLS_KERNEL_RBF_ARD>{});
    case PLS_KERNEL_MATERN12: return with_kind(integral_constant<int, PLS_KERNEL_MATERN12>{});
    case PLS_KERNEL_MATERN32: return with_kind(integral_constant<int, PLS_KERNEL_MATERN32>{});
    case PLS_KERNEL_RQ: return with_kind(integral_constant<int, PLS_KERNEL_RQ>{});
    default: return with_kind(integral_constant<int, PLS_KERNEL_MATERN52>{});
  }
}

// inv_ls[k] = sqrt(2 nu) / l_k for a stationary kind (the distance sum is then r^2 or t^2 itself; RQ keeps r^2 and divides by
// 2 alpha per pair, so that its derivative factors are the header's), 1 for the linear kernel,
// 0 for the padding k >= d: zero on both sides of a pair, so the unrolled coordinate loops need no `k < d` test.
// Periodic: inv_ls[k] = 1 / p_k (the period lengths follow the d lengthscales) and two_inv_l[k] = 2 / lambda_k, both 0 for the
// padding; the points themselves stay unscaled (pair_scaled).  The other kinds leave two_inv_l, an array of one, alone.
// Locally periodic (l, lambda, p in blocks of d): inv_env[k] = 1 / l_k, inv_ls[k] = 1 / p_k and two_inv_l[k] = 2 / lambda_k as
// for periodic, all three 0 for the padding.  Every other kind leaves inv_env, an array of one, alone.
// Trend plus seasonal (l, m, lambda, p in blocks of d, then s_s): inv_trend[k] = 1 / l_k, and the locally periodic kind's three
// arrays from (m, lambda, p), all four 0 for the padding.  Every other kind leaves inv_trend, an array of one, alone.
template <int KIND>
constexpr int periodic_len(int d_max) { return periodic_like(KIND) ? d_max : 1; }
template <int KIND>
constexpr int envelope_len(int d_max) {
  return (KIND == PLS_KERNEL_LOCALLY_PERIODIC || KIND == PLS_KERNEL_TREND_SEASONAL) ? d_max : 1;
}
template <int KIND>
constexpr int trend_len(int d_max) { return KIND == PLS_KERNEL_TREND_SEASONAL ? d_max : 1; }
template <int KIND, int D_MAX, int NP, int NE, int NT>
__device__ __forceinline__ void stage_inv_lengthscale(double (&inv_ls)[D_MAX], double (&two_inv_l)[NP], double (&inv_env)[NE],
                                                      double (&inv_trend)[NT], const double *lengthscale, int d) {
  const int t = threadIdx.x;
  if constexpr (KIND == PLS_KERNEL_TREND_SEASONAL) {
    if (t < D_MAX) {
      inv_trend[t] = (t < d) ? 1.0 / lengthscale[t] : 0.0;
      inv_env[t] = (t < d) ? 1.0 / lengthscale[d + t] : 0.0;
      two_inv_l[t] = (t < d) ? 2.0 / lengthscale[2 * d + t] : 0.0;
      inv_ls[t] = (t < d) ? 1.0 / lengthscale[3 * d + t] : 0.0;
    }
  } else if constexpr (KIND == PLS_KERNEL_LOCALLY_PERIODIC) {
    if (t < D_MAX) {
      inv_env[t] = (t < d) ? 1.0 / lengthscale[t] : 0.0;
      two_inv_l[t] = (t < d) ? 2.0 / lengthscale[d + t] : 0.0;
      inv_ls[t] = (t < d) ? 1.0 / lengthscale[2 * d + t] : 0.0;
    }
  } else if constexpr (KIND == PLS_KERNEL_PERIODIC) {
    if (t < D_MAX) {
      inv_ls[t] = (t < d) ? 1.0 / lengthscale[d + t] : 0.0;
      two_inv_l[t] = (t < d) ? 2.0 / lengthscale[t] : 0.0;
    }
  } else {
    if (t < D_MAX) inv_ls[t] = (t < d) ? ((KIND != PLS_KERNEL_LINEAR) ? matern_t_scale(KIND) / lengthscale[t] : 1.0) : 0.0;
  }
}
// a coordinate as a pairwise kernel holds it: times its inverse lengthscale, or as it is for the periodic kinds
template <int KIND>
__device__ __forceinline__ double pair_scaled(double v, double inv_ls) {
  return periodic_like(KIND) ? v : v * inv_ls;
}

// a_s[r] = row row0 + r of x (n x d, flat), pre-scaled and zero-padded, for r < nrows; 256 threads
template <int KIND, int D_MAX>
__device__ __forceinline__ void stage_rows(double (&a_s)[PAIR_ROWS][D_MAX], const double *x, int64_t row0,
                                           int nrows, int d, const double (&inv_ls)[D_MAX]) {
  for (int e = threadIdx.x; e < nrows * D_MAX; e += 256) {
    const int r = e / D_MAX, k = e % D_MAX;
    a_s[r][k] = (k < d) ? pair_scaled<KIND>(x[(row0 + r) * d + k], inv_ls[k]) : 0.0;
  }
}

// the distance sum of a staged row a and one point b, and of a and a thread's pair of columns b0, b1
template <int D_MAX>
__device__ __forceinline__ double pair_dist2(const double (&a)[D_MAX], const double (&b)[D_MAX]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    const double e = a[k] - b[k];
    s = fma(e, e, s);
  }
  return s;
}
template <int D_MAX>
__device__ __forceinline__ void pair_dist2(const double (&a)[D_MAX], const double (&b0)[D_MAX], const double (&b1)[D_MAX],
                                           double &s0, double &s1) {
  s0 = s1 = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {  // (one read of a[k] from LDS serves both columns)
    const double e0 = a[k] - b0[k], e1 = a[k] - b1[k];
    s0 = fma(e0, e0, s0);
    s1 = fma(e1, e1, s1);
  }
}

// The periodic pair loops (kernel_math.h: periodic_coord): the negated exponent of a staged row a and one point b, and of a
// and a thread's pair of columns; inv_p and two_inv_l are read from LDS (broadcast), once for both columns.
template <int D_MAX>
__device__ __forceinline__ double periodic_exponent(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                    const double (&inv_p)[D_MAX], const double (&two_inv_l)[D_MAX]) {
  double q = 0.0, unused;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) q = __dadd_rn(q, periodic_coord<false>(a[k] - b[k], inv_p[k], two_inv_l[k], unused));
  return q;
}
template <int D_MAX>
__device__ __forceinline__ void periodic_exponent(const double (&a)[D_MAX], const double (&b0)[D_MAX], const double (&b1)[D_MAX],
                                                  const double (&inv_p)[D_MAX], const double (&two_inv_l)[D_MAX], double &q0,
                                                  double &q1) {
  double unused;
  q0 = q1 = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    const double ak = a[k], ip = inv_p[k], tl = two_inv_l[k];
    q0 = __dadd_rn(q0, periodic_coord<false>(ak - b0[k], ip, tl, unused));
    q1 = __dadd_rn(q1, periodic_coord<false>(ak - b1[k], ip, tl, unused));
  }
}
// the same sum with the pair's factors kept: fl[k] = (2 / lambda_k) sin^2(pi e_k), fp[k] = (2 / lambda_k) pi e_k sin(2 pi e_k);
// dK / d log lambda_k = s kappa fl[k], dK / d log p_k = s kappa fp[k]
template <int D_MAX>
__device__ __forceinline__ double periodic_factors(const double (&a)[D_MAX], const double (&b)[D_MAX], const double (&inv_p)[D_MAX],
                                                   const double (&two_inv_l)[D_MAX], double (&fl)[D_MAX], double (&fp)[D_MAX]) {
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    fl[k] = periodic_coord<true>(a[k] - b[k], inv_p[k], two_inv_l[k], fp[k]);
    q = __dadd_rn(q, fl[k]);
  }
  return q;
}

// The locally periodic pair loops (kernel_math.h: locally_periodic_coord), laid out as the periodic ones: the negated
// exponent, each coordinate's two shares added first, then the coordinates in ascending k.
template <int D_MAX>
__device__ __forceinline__ double locally_periodic_exponent(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                            const double (&inv_l)[D_MAX], const double (&inv_p)[D_MAX],
                                                            const double (&two_inv_lam)[D_MAX]) {
  double q = 0.0, u0, u1, u2;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k)
    q = __dadd_rn(q, locally_periodic_coord<false>(a[k] - b[k], inv_l[k], inv_p[k], two_inv_lam[k], u0, u1, u2));
  return q;
}
template <int D_MAX>
__device__ __forceinline__ void locally_periodic_exponent(const double (&a)[D_MAX], const double (&b0)[D_MAX],
                                                          const double (&b1)[D_MAX], const double (&inv_l)[D_MAX],
                                                          const double (&inv_p)[D_MAX], const double (&two_inv_lam)[D_MAX],
                                                          double &q0, double &q1) {
  double u0, u1, u2;
  q0 = q1 = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    const double ak = a[k], il = inv_l[k], ip = inv_p[k], tl = two_inv_lam[k];
    q0 = __dadd_rn(q0, locally_periodic_coord<false>(ak - b0[k], il, ip, tl, u0, u1, u2));
    q1 = __dadd_rn(q1, locally_periodic_coord<false>(ak - b1[k], il, ip, tl, u0, u1, u2));
  }
}
// The reduction keeps the factors of a column's first KEEP coordinates between the exponent sum and the accumulation and
// evaluates the others a second time afterwards (the same function of the same operands: the same bits), so that at
// D_MAX = 16 no more than 24 factors are live beside the 49 accumulators.
constexpr int locally_periodic_keep(int d_max) { return d_max > 8 ? d_max / 2 : d_max; }
// the same sum with the factors of the coordinates k < KEEP kept: fe[k] = ((a_k - b_k) / l_k)^2, fl[k] and fp[k] as
// periodic_factors'; dK / d log l_k = s kappa fe[k], dK / d log lambda_k = s kappa fl[k], dK / d log p_k = s kappa fp[k]
template <int D_MAX, int KEEP>
__device__ __forceinline__ double locally_periodic_factors(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                           const double (&inv_l)[D_MAX], const double (&inv_p)[D_MAX],
                                                           const double (&two_inv_lam)[D_MAX], double (&fe)[KEEP],
                                                           double (&fl)[KEEP], double (&fp)[KEEP]) {
  double q = 0.0, u0, u1, u2;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    if (k < KEEP)
      q = __dadd_rn(q, locally_periodic_coord<true>(a[k] - b[k], inv_l[k], inv_p[k], two_inv_lam[k], fe[k % KEEP], fl[k % KEEP],
                                                    fp[k % KEEP]));
    else
      q = __dadd_rn(q, locally_periodic_coord<false>(a[k] - b[k], inv_l[k], inv_p[k], two_inv_lam[k], u0, u1, u2));
  }
  return q;
}

// The trend-plus-seasonal pair loops (kernel_math.h: trend_seasonal_coord), laid out as the locally periodic ones: q, the
// seasonal term's negated exponent, is locally_periodic_exponent's of (inv_m, inv_p, two_inv_lam) bit for bit; s, the trend's
// distance sum, is accumulated beside it from the same differences, in ascending k.
template <int D_MAX>
__device__ __forceinline__ void trend_seasonal_exponents(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                         const double (&inv_t)[D_MAX], const double (&inv_m)[D_MAX],
                                                         const double (&inv_p)[D_MAX], const double (&two_inv_lam)[D_MAX],
                                                         double &s, double &q) {
  double u0, u1, u2, u3;
  s = q = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k)
    q = __dadd_rn(q, trend_seasonal_coord<false>(a[k] - b[k], inv_t[k], inv_m[k], inv_p[k], two_inv_lam[k], s, u0, u1, u2, u3));
}
template <int D_MAX>
__device__ __forceinline__ void trend_seasonal_exponents(const double (&a)[D_MAX], const double (&b0)[D_MAX],
                                                         const double (&b1)[D_MAX], const double (&inv_t)[D_MAX],
                                                         const double (&inv_m)[D_MAX], const double (&inv_p)[D_MAX],
                                                         const double (&two_inv_lam)[D_MAX], double &s0, double &q0, double &s1,
                                                         double &q1) {
  double u0, u1, u2, u3;
  s0 = q0 = s1 = q1 = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    const double ak = a[k], it = inv_t[k], im = inv_m[k], ip = inv_p[k], tl = two_inv_lam[k];
    q0 = __dadd_rn(q0, trend_seasonal_coord<false>(ak - b0[k], it, im, ip, tl, s0, u0, u1, u2, u3));
    q1 = __dadd_rn(q1, trend_seasonal_coord<false>(ak - b1[k], it, im, ip, tl, s1, u0, u1, u2, u3));
  }
}
// the same two sums with the pair's factors kept: ft[k] = ((a_k - b_k) / l_k)^2, dK / d log l_k = s_t kappa_t ft[k]; fe, fl and
// fp as locally_periodic_factors', dK / d log m_k, lambda_k, p_k = s_s kappa_s fe[k], fl[k], fp[k]
template <int D_MAX>
__device__ __forceinline__ void trend_seasonal_factors(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                       const double (&inv_t)[D_MAX], const double (&inv_m)[D_MAX],
                                                       const double (&inv_p)[D_MAX], const double (&two_inv_lam)[D_MAX],
                                                       double &s, double &q, double (&ft)[D_MAX], double (&fe)[D_MAX],
                                                       double (&fl)[D_MAX], double (&fp)[D_MAX]) {
  s = q = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k)
    q = __dadd_rn(q, trend_seasonal_coord<true>(a[k] - b[k], inv_t[k], inv_m[k], inv_p[k], two_inv_lam[k], s, ft[k], fe[k], fl[k],
                                                fp[k]));
}

}  // namespace plship
