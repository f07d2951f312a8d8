// What the pairwise kernels of base_kernel.hip share (Gram build, gradient reduction, fused predictive mean): tile geometry,
// the table of kind facts and what follows from it, the staging of the scales and of the points, the loops over the
// coordinates of a pair, the KIND x D_MAX dispatch.  The pair's value: kernel_math.h.
// Two schemes.  A distance-sum kind (RBF, Matern, RQ) stages its points times 1 / l_k and evaluates a pair from one sum of
// squares (pair_dist2).  A per-coordinate kind (periodic, locally periodic, trend plus seasonal) stages its points UNSCALED,
// keeps one scale per coordinate and parameter block in LDS, and evaluates every coordinate on its own (kernel_math.h:
// pair_coord; here pair_exponents and pair_factors_kept).  Such a kind is its row of kind_facts, its coordinate function and
// its entry function (kernel_math.h); everything else in this file and in base_kernel.hip is derived from the row.
#pragma once
#include "common.h"
#include "kernel_math.h"

namespace plship {

// A workgroup of the Gram build or of the reduction covers PAIR_ROWS rows x PAIR_COLS columns of the pair matrix: 256
// threads, a pair of columns each, walking down the rows.  PAIR_D_MAX: the largest input dimension of every pairwise kernel.
constexpr int PAIR_ROWS = 64, PAIR_COLS = 512, PAIR_D_MAX = 64;

// What the library knows of a kernel kind.  Its `lengthscale` argument holds the d lengthscales, then `blocks` blocks of d
// values, then `scalars` values: RQ alpha; periodic lambda | p (the lengthscales ARE lambda); locally periodic l | lambda | p;
// trend plus seasonal l | m | lambda | p, then s_s.
// d_max: the reduction carries (1 + blocks) D_MAX + 1 + scalars accumulators per thread -- periodic 33 at 16, what RBF carries
// at 32; locally periodic 49 at 16; trend plus seasonal 34 at 8, and it would carry 66 beside the factors at 16.
struct KindFacts {
  int blocks;        // per-dimension blocks behind the d lengthscales
  int scalars;       // scalars behind those blocks
  int d_max;         // the largest input dimension
  bool per_coord;    // points staged unscaled, every coordinate evaluated on its own
  int terms;         // kappas of a pair, each with its own outputscale and underflow decision; 0: not a kind
  const char *noun;  // of check_kind_dim's message, where d_max is the kind's own
};
constexpr KindFacts kind_facts(int kind) {
  switch (kind) {
    case PLS_KERNEL_RBF_ARD:
    case PLS_KERNEL_LINEAR:
    case PLS_KERNEL_MATERN12:
    case PLS_KERNEL_MATERN32:
    case PLS_KERNEL_MATERN52: return {0, 0, PAIR_D_MAX, false, 1, nullptr};
    case PLS_KERNEL_RQ: return {0, 1, PAIR_D_MAX, false, 1, nullptr};
    case PLS_KERNEL_PERIODIC: return {1, 0, 16, true, 1, "periodic"};
    case PLS_KERNEL_LOCALLY_PERIODIC: return {2, 0, 16, true, 1, "locally periodic"};
    case PLS_KERNEL_TREND_SEASONAL: return {3, 1, 8, true, 2, "trend-plus-seasonal"};
    default: return {0, 0, PAIR_D_MAX, false, 0, nullptr};
  }
}
constexpr bool periodic_like(int kind) { return kind_facts(kind).per_coord; }
static inline int64_t kind_d_max(int32_t kind) { return kind_facts(kind).d_max; }
// rows of a kind's scale block in LDS: one per parameter block of a per-coordinate kind, else the one of 1 / l_k
constexpr int scale_rows(int kind) { return periodic_like(kind) ? 1 + kind_facts(kind).blocks : 1; }

// pls_kernel_mean: test points of a workgroup (one per lane, the four waves split the training points), and the training
// points staged in LDS at a time: 32 KiB of pre-scaled coordinates, 512 points at the most; a multiple of 4 for every D_MAX
constexpr int MEAN_POINTS = 64;
constexpr int mean_chunk(int d_max) { return 4096 / d_max < 512 ? 4096 / d_max : 512; }

// shape parameters of a kind: what follows the d lengthscales in its `lengthscale` argument
static inline int64_t kind_shape_params(int32_t kind, int64_t d) { return kind_facts(kind).blocks * d + kind_facts(kind).scalars; }
// sums of the reduction: the kappa sum, one per lengthscale, one per shape parameter
static inline int64_t grad_sums_count(int32_t kind, int64_t d) { return d + 1 + kind_shape_params(kind, d); }

// workgroups of the reduction over an n x n matrix = partial rows of grad_sums_count doubles in its workspace
static inline int64_t grad_sums_blocks(int64_t n) { return cdiv(n, PAIR_COLS) * cdiv(n, PAIR_ROWS); }
static inline size_t grad_sums_workspace_bytes(int32_t kind, int64_t n, int64_t d) {
  return (size_t)grad_sums_blocks(n) * (size_t)grad_sums_count(kind, d) * sizeof(double);
}

static inline bool stationary_kind(int32_t kind) { return kind != PLS_KERNEL_LINEAR && kind_facts(kind).terms > 0; }
// what every entry checks after the kind and d >= 1: the kind's largest input dimension, under the entry's name `who`
static inline int check_kind_dim(const char *who, int32_t kind, int64_t d) {
  const KindFacts f = kind_facts(kind);
  PLS_REQUIRE(d <= f.d_max, "%s: input dimension %lld > %d is not supported%s%s%s", who, (long long)d, f.d_max,
              f.noun ? " for the " : "", f.noun ? f.noun : "", f.noun ? " kernel" : "");
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
// the input dimension rounded up to 1, 2, 4, ..., the kind's d_max (kind and d already validated).  LINEAR: with the linear
// kind (the Gram build).
template <int D_MAX, class K, class F>
static int for_dmax_from(int d, K k, F &&f) {
  if constexpr (D_MAX < kind_facts(K::value).d_max)
    if (d > D_MAX) return for_dmax_from<2 * D_MAX>(d, k, f);
  return f(k, std::integral_constant<int, D_MAX>{});
}
template <bool LINEAR, class F>
static int for_kind_dmax(int kind, int d, F &&f) {
  using std::integral_constant;
  if constexpr (LINEAR)
    if (kind == PLS_KERNEL_LINEAR) return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_LINEAR>{}, f);
  switch (kind) {
    case PLS_KERNEL_RBF_ARD: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_RBF_ARD>{}, f);
    case PLS_KERNEL_MATERN12: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_MATERN12>{}, f);
    case PLS_KERNEL_MATERN32: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_MATERN32>{}, f);
    case PLS_KERNEL_RQ: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_RQ>{}, f);
    case PLS_KERNEL_PERIODIC: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_PERIODIC>{}, f);
    case PLS_KERNEL_LOCALLY_PERIODIC: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_LOCALLY_PERIODIC>{}, f);
    case PLS_KERNEL_TREND_SEASONAL: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_TREND_SEASONAL>{}, f);
    default: return for_dmax_from<1>(d, integral_constant<int, PLS_KERNEL_MATERN52>{}, f);
  }
}

// The scale block of a workgroup, scale_rows(KIND) rows of D_MAX, and the only statement of what it holds: row j is block j of
// the `lengthscale` argument as numerator / value, 0 for the padding k >= d -- zero on both sides of a pair, so the unrolled
// coordinate loops need no `k < d` test.  Distance-sum kinds: sqrt(2 nu) / l_k (the distance sum is then r^2 or t^2 itself; RQ
// keeps r^2 and divides by 2 alpha per pair, so that its derivative factors are the header's); the linear kernel: 1.
// Per-coordinate kinds: 2 over lambda_k, the last block but one, and 1 over every other value (kernel_math.h: pair_coord).
template <int KIND, int D_MAX>
__device__ __forceinline__ void stage_scales(double (&scales)[scale_rows(KIND)][D_MAX], const double *lengthscale, int d) {
  constexpr int NS = scale_rows(KIND);
  const int t = threadIdx.x;
  if (t < D_MAX) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const double numerator = periodic_like(KIND) ? (j == NS - 2 ? 2.0 : 1.0) : matern_t_scale(KIND);
      scales[j][t] = (t < d) ? ((KIND != PLS_KERNEL_LINEAR) ? numerator / lengthscale[j * d + t] : 1.0) : 0.0;
    }
  }
}
// a coordinate as a pairwise kernel holds it: times its inverse lengthscale, or as it is for the per-coordinate kinds
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

// The coordinate loops of the per-coordinate kinds (kernel_math.h: pair_coord): q, the negated exponent, and s, the trend's
// distance sum (0 where the kind has none), both added in ascending k, of a staged row a and one point b, and of a and a
// thread's pair of columns; a[k] and column k of the scales are read from LDS (broadcast) once for both columns.
template <int NS, int D_MAX>
__device__ __forceinline__ void scale_column(const double (&scales)[NS][D_MAX], int k, double (&sc)[NS]) {
#pragma unroll
  for (int j = 0; j < NS; ++j) sc[j] = scales[j][k];
}
template <int KIND, int NS, int D_MAX>
__device__ __forceinline__ void pair_exponents(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                               const double (&scales)[NS][D_MAX], double &s, double &q) {
  double sc[NS], unused[NS];
  s = q = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    scale_column(scales, k, sc);
    q = __dadd_rn(q, pair_coord<KIND, false>(a[k] - b[k], sc, s, unused));
  }
}
template <int KIND, int NS, int D_MAX>
__device__ __forceinline__ void pair_exponents(const double (&a)[D_MAX], const double (&b0)[D_MAX], const double (&b1)[D_MAX],
                                               const double (&scales)[NS][D_MAX], double &s0, double &q0, double &s1,
                                               double &q1) {
  double sc[NS], unused[NS];
  s0 = q0 = s1 = q1 = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    const double ak = a[k];
    scale_column(scales, k, sc);
    q0 = __dadd_rn(q0, pair_coord<KIND, false>(ak - b0[k], sc, s0, unused));
    q1 = __dadd_rn(q1, pair_coord<KIND, false>(ak - b1[k], sc, s1, unused));
  }
}
// The reduction keeps the factors of a column's first KEEP coordinates between the sums and the accumulation and evaluates
// the others a second time afterwards (the same function of the same operands: the same bits), so that no more than 32
// factors are live beside the accumulators: every coordinate's except at locally periodic's D_MAX = 16, 24 beside 49.
constexpr int factors_kept(int kind, int d_max) { return scale_rows(kind) * d_max > 32 ? d_max / 2 : d_max; }
// the same sums with the factors of the coordinates k < KEEP kept: f[j][k], coordinate k's factor of dK / d log of block j's
// parameter (kernel_math.h: pair_coord)
template <int KIND, int KEEP, int NS, int D_MAX>
__device__ __forceinline__ void pair_factors_kept(const double (&a)[D_MAX], const double (&b)[D_MAX],
                                                  const double (&scales)[NS][D_MAX], double &s, double &q,
                                                  double (&f)[NS][KEEP]) {
  double sc[NS], fk[NS];
  s = q = 0.0;
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    scale_column(scales, k, sc);
    if (k < KEEP) {
      q = __dadd_rn(q, pair_coord<KIND, true>(a[k] - b[k], sc, s, fk));
#pragma unroll
      for (int j = 0; j < NS; ++j) f[j][k % KEEP] = fk[j];
    } else {
      q = __dadd_rn(q, pair_coord<KIND, false>(a[k] - b[k], sc, s, fk));
    }
  }
}

}  // namespace plship
