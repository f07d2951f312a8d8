// What the pairwise kernels of base_kernel.hip share (Gram build, gradient reduction, fused predictive mean): tile geometry,
// the pre-scaled staging of the points, the distance sum of a pair, the KIND x D_MAX dispatch.  The pair's value: kernel_math.h.
#pragma once
#include "common.h"
#include "kernel_math.h"

namespace plship {

// A workgroup of the Gram build or of the reduction covers PAIR_ROWS rows x PAIR_COLS columns of the pair matrix: 256
// threads, a pair of columns each, walking down the rows.  PAIR_D_MAX: the largest input dimension of every pairwise kernel.
constexpr int PAIR_ROWS = 64, PAIR_COLS = 512, PAIR_D_MAX = 64;

// pls_kernel_mean: test points of a workgroup (one per lane, the four waves split the training points), and the training
// points staged in LDS at a time: 32 KiB of pre-scaled coordinates, 512 points at the most; a multiple of 4 for every D_MAX
constexpr int MEAN_POINTS = 64;
constexpr int mean_chunk(int d_max) { return 4096 / d_max < 512 ? 4096 / d_max : 512; }

// shape parameters of a kind: they follow the d lengthscales in its `lengthscale` argument (RQ: alpha)
static inline int64_t kind_shape_params(int32_t kind) { return kind == PLS_KERNEL_RQ ? 1 : 0; }
// sums of the reduction: the kappa sum, one per lengthscale, one per shape parameter
static inline int64_t grad_sums_count(int32_t kind, int64_t d) { return d + 1 + kind_shape_params(kind); }

// workgroups of the reduction over an n x n matrix = partial rows of grad_sums_count doubles in its workspace
static inline int64_t grad_sums_blocks(int64_t n) { return cdiv(n, PAIR_COLS) * cdiv(n, PAIR_ROWS); }
static inline size_t grad_sums_workspace_bytes(int32_t kind, int64_t n, int64_t d) {
  return (size_t)grad_sums_blocks(n) * (size_t)grad_sums_count(kind, d) * sizeof(double);
}

static inline bool stationary_kind(int32_t kind) {
  return kind == PLS_KERNEL_RBF_ARD || kind == PLS_KERNEL_MATERN12 || kind == PLS_KERNEL_MATERN32 || kind == PLS_KERNEL_MATERN52 ||
         kind == PLS_KERNEL_RQ;
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
// the input dimension rounded up to 1, 2, 4, ..., 64 (kind and d already validated).  LINEAR: with the linear kind (the Gram build).
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
template <int KIND, int D_MAX>
__device__ __forceinline__ void stage_inv_lengthscale(double (&inv_ls)[D_MAX], const double *lengthscale, int d) {
  const int t = threadIdx.x;
  if (t < D_MAX) inv_ls[t] = (t < d) ? ((KIND != PLS_KERNEL_LINEAR) ? matern_t_scale(KIND) / lengthscale[t] : 1.0) : 0.0;
}

// a_s[r] = row row0 + r of x (n x d, flat), pre-scaled and zero-padded, for r < nrows; 256 threads
template <int D_MAX>
__device__ __forceinline__ void stage_rows(double (&a_s)[PAIR_ROWS][D_MAX], const double *x, int64_t row0,
                                           int nrows, int d, const double (&inv_ls)[D_MAX]) {
  for (int e = threadIdx.x; e < nrows * D_MAX; e += 256) {
    const int r = e / D_MAX, k = e % D_MAX;
    a_s[r][k] = (k < d) ? x[(row0 + r) * d + k] * inv_ls[k] : 0.0;
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

}  // namespace plship
