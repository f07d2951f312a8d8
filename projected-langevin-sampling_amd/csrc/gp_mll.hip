// Exact-GP marginal log-likelihood and its gradient with respect to the base-kernel hyper-parameters.
//
// Reference: mll(model(x), y) and loss.backward() of train_exact_gp (experiments/trainers.py:45-49), i.e. gpytorch's
// ExactMarginalLogLikelihood of ScaleKernel(RBFKernel | MaternKernel) + GaussianLikelihood with a constant mean.
//
//   K_y = s kappa(x, x) + (noise + jitter) I = Lc Lc^T,   r = y - mean,   alpha = K_y^-1 r,   W = alpha alpha^T - K_y^-1
//   mll = -1/2 r^T alpha - sum_i log Lc_ii - n/2 log 2 pi,                d mll / d theta = 1/2 sum_ij W_ij dK_ij / d theta
//
// The Gram build, the factorisation, the solve, the inverse factor and K_y^-1 = Linv^T Linv are the library's existing
// kernels.  New here is the reduction over all n^2 pairs, kernel_grad_sums_kernel: one pass over P (= K_y^-1) that
// recomputes kappa and its lengthscale derivatives from x and leaves d + 1 sums,
//   out[0]     = sum_ij W_ij kappa_ij                  (kappa: the kernel without its outputscale)
//   out[1 + k] = sum_ij W_ij dK_ij / d log l_k         (RBF: s exp(-r^2/2) e_k^2;  Matern: s q(t) exp(-t) 2 nu e_k^2 with
//                                                       q = 1/t, 1, (1 + t)/3 for nu = 1/2, 3/2, 5/2;  e_k = (x_ik - x_jk)/l_k)
// in a fixed summation order: per thread down the rows of its column pair, xor butterfly inside each wave, (w0 + w1) +
// (w2 + w3) per workgroup, the workgroups' partial rows in ascending order (a second one-workgroup launch).  No atomics.
//
// Classification (gpytorch's DirichletClassificationLikelihood, Milios et al. 2018): one such GP per class on the shared
// x, K_y,c = s_c kappa(x, x; l_c) + diag(v_c) + sigma_c I with a fixed noise v_c per point -- pls_gp_mll_grad_classes runs
// the same evaluation per class with the diagonal as a vector (add_diag_vector_kernel); softmax_normal_mean_kernel turns
// the latent means and variances at test points into class probabilities on the library's Philox stream.
#include <hip/hip_runtime.h>

#define PLS_SCALAR_POLY_CONSTANTS 1  // (fmath.h: the exp polynomial's constants as scalar operands, as in the Gram build)
#include "../../include/plship.h"
#include "chol.h"
#include "common.h"
#include "gemm_api.h"
#include "gp_mll.h"
#include "kernel_math.h"
#include "philox.h"

namespace plship {

typedef double double2m __attribute__((ext_vector_type(2)));

// One pair from its distance sum s2 (RBF: r^2; Matern: t^2 = 2 nu r^2, the inverse lengthscales carry sqrt(2 nu)):
//   kap = kappa_ij;  g: dK_ij / d log l_k = outputscale * g * e'_k^2 with e'_k the pre-scaled difference;
//   returns false for a pair whose exponential underflows -- the caller skips it, so that it contributes exactly 0 (its
//   e'_k^2 may be inf: 0 * inf would be NaN).
template <int KIND>
__device__ __forceinline__ bool pair_factors(double s2, double &kap, double &g) {
  if (KIND == PLS_KERNEL_RBF_ARD) {
    kap = g = exp_nonpos_unguarded(-0.5 * s2);
    return !(s2 > 1490.4);
  }
  const double t = sqrt(s2);
  const double ex = exp_nonpos_unguarded(-t);
  kap = matern_poly(KIND, t) * ex;
  if (KIND == PLS_KERNEL_MATERN12) g = (t > 0.0) ? ex / t : 0.0;  // r = 0: every e_k is 0 and the pair contributes 0
  else if (KIND == PLS_KERNEL_MATERN32) g = ex;
  else g = ex * ((1.0 + t) * (1.0 / 3.0));
  return !(t > 745.2);
}

// A workgroup covers GRAD_ROWS rows x GRAD_COLS columns of the n x n pair matrix, laid out as kernel_gram_kernel: a
// thread owns a PAIR of columns (its two points stay in registers, pre-scaled by 1/lengthscale) and walks down the rows,
// whose pre-scaled points sit in LDS (broadcast reads).  P is read once, 16 B per lane where ldp is even and P is
// 16-byte aligned.  D_MAX + 1 accumulators per thread; the padding coordinates are zero on both sides.
template <int KIND, int D_MAX>
__global__ __launch_bounds__(256) void kernel_grad_sums_kernel(const double *__restrict__ x, int64_t n, int d,
                                                                const double *__restrict__ lengthscale, double outputscale,
                                                                const double *__restrict__ alpha, const double *__restrict__ P,
                                                                int64_t ldp, double *__restrict__ partials) {
  __shared__ double inv_ls[D_MAX];
  __shared__ __attribute__((aligned(16))) double a_s[GRAD_ROWS][D_MAX];
  __shared__ double al_s[GRAD_ROWS];
  __shared__ double red[4][D_MAX + 1];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * GRAD_ROWS;
  const int nrows = (int)((n - row0 < GRAD_ROWS) ? (n - row0) : GRAD_ROWS);
  if (t < D_MAX) inv_ls[t] = (t < d) ? matern_t_scale(KIND) / lengthscale[t] : 0.0;
  if (t < GRAD_ROWS) al_s[t] = (t < nrows) ? alpha[row0 + t] : 0.0;
  __syncthreads();
  for (int e = t; e < nrows * D_MAX; e += 256) {
    const int r = e / D_MAX, k = e % D_MAX;
    a_s[r][k] = (k < d) ? x[(row0 + r) * d + k] * inv_ls[k] : 0.0;
  }
  __syncthreads();
  const int64_t col = ((int64_t)blockIdx.x * 256 + t) * 2;
  const bool one = col < n, two = col + 1 < n;
  double acc[D_MAX + 1];
#pragma unroll
  for (int k = 0; k <= D_MAX; ++k) acc[k] = 0.0;
  if (one) {
    double b0[D_MAX], b1[D_MAX];
#pragma unroll
    for (int k = 0; k < D_MAX; ++k) {
      b0[k] = (k < d) ? x[col * d + k] * inv_ls[k] : 0.0;
      b1[k] = (k < d && two) ? x[(col + 1) * d + k] * inv_ls[k] : 0.0;
    }
    const double aj0 = alpha[col], aj1 = two ? alpha[col + 1] : 0.0;
    const bool vec = two && ((ldp & 1) == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0);
    const double *src = P + row0 * ldp + col;
    for (int r = 0; r < nrows; ++r, src += ldp) {
      double p0, p1 = 0.0;
      if (vec) {
        const double2m v = *reinterpret_cast<const double2m *>(src);
        p0 = v.x;
        p1 = v.y;
      } else {
        p0 = src[0];
        if (two) p1 = src[1];
      }
      const double ai = al_s[r];
      const double w0 = __dsub_rn(__dmul_rn(ai, aj0), p0), w1 = __dsub_rn(__dmul_rn(ai, aj1), p1);  // W_ij, two roundings
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int k = 0; k < D_MAX; ++k) {
        const double a = a_s[r][k];
        const double e0 = a - b0[k], e1 = a - b1[k];
        s0 = fma(e0, e0, s0);
        s1 = fma(e1, e1, s1);
      }
      double kap0, g0, kap1, g1;
      const bool live0 = pair_factors<KIND>(s0, kap0, g0);
      const bool live1 = pair_factors<KIND>(s1, kap1, g1) && two;
      if (live0) {
        const double gw = w0 * (outputscale * g0);
        acc[0] = fma(w0, kap0, acc[0]);
#pragma unroll
        for (int k = 0; k < D_MAX; ++k) {
          const double e = a_s[r][k] - b0[k];
          acc[1 + k] = fma(gw, e * e, acc[1 + k]);
        }
      }
      if (live1) {
        const double gw = w1 * (outputscale * g1);
        acc[0] = fma(w1, kap1, acc[0]);
#pragma unroll
        for (int k = 0; k < D_MAX; ++k) {
          const double e = a_s[r][k] - b1[k];
          acc[1 + k] = fma(gw, e * e, acc[1 + k]);
        }
      }
    }
  }
  // workgroup sum in a fixed order: xor butterfly inside each wave, then (w0 + w1) + (w2 + w3)
#pragma unroll
  for (int k = 0; k <= D_MAX; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((t & 63) == 0) red[t >> 6][k] = v;
  }
  __syncthreads();
  if (t <= d) {
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * (d + 1) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

// out[k] = the partial rows of the workgroups added in ascending order
__global__ __launch_bounds__(128) void grad_sums_finish_kernel(const double *__restrict__ partials, int64_t nblocks, int d,
                                                                double *__restrict__ out) {
  const int k = threadIdx.x;
  if (k > d) return;
  double s = 0.0;
  for (int64_t b = 0; b < nblocks; ++b) s += partials[b * (d + 1) + k];
  out[k] = s;
}

template <int KIND>
static void launch_grad_sums(dim3 grid, hipStream_t st, const double *x, int64_t n, int d, const double *lengthscale,
                             double outputscale, const double *alpha, const double *P, int64_t ldp, double *partials) {
#define PLS_GRAD_CASE(DM)                                                                                          \
  hipLaunchKernelGGL((kernel_grad_sums_kernel<KIND, DM>), grid, dim3(256), 0, st, x, n, d, lengthscale, outputscale, \
                     alpha, P, ldp, partials)
  if (d <= 1) PLS_GRAD_CASE(1);
  else if (d <= 2) PLS_GRAD_CASE(2);
  else if (d <= 4) PLS_GRAD_CASE(4);
  else if (d <= 8) PLS_GRAD_CASE(8);
  else if (d <= 16) PLS_GRAD_CASE(16);
  else if (d <= 32) PLS_GRAD_CASE(32);
  else PLS_GRAD_CASE(64);
#undef PLS_GRAD_CASE
}

static size_t grad_sums_workspace_bytes(int64_t n, int64_t d) { return (size_t)grad_sums_blocks(n) * (size_t)(d + 1) * sizeof(double); }

// the reduction and its finishing launch (arguments already validated)
static int grad_sums_launch(int kind, const double *x, int64_t n, int d, const double *lengthscale, double outputscale,
                            const double *alpha, const double *P, int64_t ldp, double *out, double *partials, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(n, GRAD_COLS), (unsigned)cdiv(n, GRAD_ROWS));
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    switch (kind) {
      case PLS_KERNEL_RBF_ARD: launch_grad_sums<PLS_KERNEL_RBF_ARD>(grid, st, x, n, d, lengthscale, outputscale, alpha, P, ldp, partials); break;
      case PLS_KERNEL_MATERN12: launch_grad_sums<PLS_KERNEL_MATERN12>(grid, st, x, n, d, lengthscale, outputscale, alpha, P, ldp, partials); break;
      case PLS_KERNEL_MATERN32: launch_grad_sums<PLS_KERNEL_MATERN32>(grid, st, x, n, d, lengthscale, outputscale, alpha, P, ldp, partials); break;
      default: launch_grad_sums<PLS_KERNEL_MATERN52>(grid, st, x, n, d, lengthscale, outputscale, alpha, P, ldp, partials); break;
    }
  }
  if (int rc = check_launch("kernel_grad_sums")) return rc;
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(grad_sums_finish_kernel, dim3(1), dim3(128), 0, st, partials, grad_sums_blocks(n), d, out);
  }
  return check_launch("grad_sums_finish");
}

// ---- the predictive mean without the cross-Gram matrix -------------------------------------------------------------
// kappa (the kernel without its outputscale) of one pair from its distance sum s2, evaluated as kernel_gram_kernel
// evaluates it (plship.hip); false for a pair whose exponential underflows: the caller skips it (exactly 0).
template <int KIND>
__device__ __forceinline__ bool pair_kappa(double s2, double &kap) {
  if (KIND == PLS_KERNEL_RBF_ARD) {
    kap = exp_nonpos_unguarded(-0.5 * s2);
    return !(-0.5 * s2 < -745.2);
  }
  const double t = sqrt(s2);
  kap = matern_poly(KIND, t) * exp_nonpos_unguarded(-t);
  return !(t > 745.2);
}

// out[i] = mean + outputscale * sum_j kappa(xt_i, x_j) alpha_j.  A workgroup owns MEAN_POINTS = 64 test points: lane l of
// EVERY wave holds test point 64 b + l in registers (pre-scaled by 1/lengthscale, zero-padded to D_MAX); the training
// points pass through LDS in chunks of mean_chunk(D_MAX) (pre-scaled, broadcast reads) and wave w takes the points
// j = w, w + 4, w + 8, ... (the chunk length is a multiple of 4, so the split is j mod 4 whatever the chunk).  Each thread
// adds its terms in ascending j into one accumulator; the four waves' sums meet in LDS as (w0 + w1) + (w2 + w3).  A lane
// owns its test point alone -- there is no cross-lane sum -- so out[i] depends on xt_i and the model only, never on t or
// on where the point sits in the batch.  x is staged from its flat array, 16 bytes per lane where x is 16-byte aligned
// (a chunk starts at an even offset), one double per lane otherwise; xt rows likewise where d is even.
template <int KIND, int D_MAX>
__global__ __launch_bounds__(256) void kernel_mean_kernel(const double *__restrict__ x, int64_t n, int d,
                                                           const double *__restrict__ lengthscale, double outputscale,
                                                           double mean, const double *__restrict__ alpha,
                                                           const double *__restrict__ xt, int64_t t,
                                                           double *__restrict__ out) {
  constexpr int CHUNK = mean_chunk(D_MAX);
  __shared__ double inv_ls[D_MAX];
  __shared__ __attribute__((aligned(16))) double a_s[CHUNK][D_MAX];
  __shared__ double al_s[CHUNK];
  __shared__ double red[4][MEAN_POINTS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < D_MAX) inv_ls[tid] = (tid < d) ? matern_t_scale(KIND) / lengthscale[tid] : 0.0;
  if (D_MAX > 1)  // the padding coordinates stay zero: the staging below writes k < d only
    for (int e = tid; e < CHUNK * D_MAX; e += 256) a_s[e / D_MAX][e % D_MAX] = 0.0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * MEAN_POINTS + lane;
  const bool live = i < t;
  double b[D_MAX];
  {
    const double *row = xt + (live ? i : 0) * d;
    if ((d & 1) == 0 && (reinterpret_cast<uintptr_t>(xt) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < D_MAX; k += 2) {
        const double2m v = (k < d) ? *reinterpret_cast<const double2m *>(row + k) : double2m{0.0, 0.0};
        b[k] = v.x * inv_ls[k];
        if (k + 1 < D_MAX) b[k + 1] = v.y * inv_ls[(k + 1) % D_MAX];
      }
    } else {
#pragma unroll
      for (int k = 0; k < D_MAX; ++k) b[k] = (k < d) ? row[k] * inv_ls[k] : 0.0;
    }
  }
  const bool xvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  double acc = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += CHUNK) {
    const int nrows = (int)((n - j0 < CHUNK) ? (n - j0) : CHUNK);
    const int len = nrows * d;  // <= 512 * 64
    const double *src = x + j0 * d;
    if (xvec) {
      for (int p = tid; 2 * p < len; p += 256) {
        const int e = 2 * p;
        if (e + 1 < len) {
          const double2m v = *reinterpret_cast<const double2m *>(src + e);
          a_s[e / d][e % d] = v.x * inv_ls[e % d];
          a_s[(e + 1) / d][(e + 1) % d] = v.y * inv_ls[(e + 1) % d];
        } else {
          a_s[e / d][e % d] = src[e] * inv_ls[e % d];
        }
      }
    } else {
      for (int e = tid; e < len; e += 256) a_s[e / d][e % d] = src[e] * inv_ls[e % d];
    }
    for (int r = tid; r < nrows; r += 256) al_s[r] = alpha[j0 + r];
    __syncthreads();
#pragma unroll 2
    for (int r = w; r < nrows; r += 4) {
      double s2 = 0.0;
#pragma unroll
      for (int k = 0; k < D_MAX; ++k) {
        const double e = a_s[r][k] - b[k];
        s2 = fma(e, e, s2);
      }
      double kap;
      if (pair_kappa<KIND>(s2, kap)) acc = fma(kap, al_s[r], acc);
    }
    __syncthreads();
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0 && live) out[i] = fma(outputscale, (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]), mean);
}

// The KIND x D_MAX instantiations of a stationary kernel's per-pair loops: f(integral_constant<KIND>, integral_constant<D_MAX>)
// with D_MAX the input dimension rounded up to 1, 2, 4, 8, 16, 32 or 64 (kind and d already validated).
template <class F>
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
  switch (kind) {
    case PLS_KERNEL_RBF_ARD: return with_kind(integral_constant<int, PLS_KERNEL_RBF_ARD>{});
    case PLS_KERNEL_MATERN12: return with_kind(integral_constant<int, PLS_KERNEL_MATERN12>{});
    case PLS_KERNEL_MATERN32: return with_kind(integral_constant<int, PLS_KERNEL_MATERN32>{});
    default: return with_kind(integral_constant<int, PLS_KERNEL_MATERN52>{});
  }
}

// the one launch of pls_kernel_mean (arguments already validated, t > 0)
static int kernel_mean_launch(int kind, const double *x, int64_t n, int d, const double *lengthscale, double outputscale,
                              double mean, const double *alpha, const double *xt, int64_t t, double *out, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(t, (int64_t)MEAN_POINTS));
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    for_kind_dmax(kind, d, [&](auto k, auto dm) {
      hipLaunchKernelGGL((kernel_mean_kernel<decltype(k)::value, decltype(dm)::value>), grid, dim3(256), 0, st, x, n, d,
                         lengthscale, outputscale, mean, alpha, xt, t, out);
      return 0;
    });
  }
  return check_launch("kernel_mean");
}

// r = y - mean
__global__ __launch_bounds__(256) void gp_center_kernel(const double *__restrict__ y, double mean, int64_t n, double *__restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) r[i] = y[i] - mean;
}

// workgroup sum of one value per thread in the library's fixed order; every thread returns the total
__device__ __forceinline__ double block256_sum(double v, double (*ws)[4], int slot) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) ws[slot][threadIdx.x >> 6] = v;
  __syncthreads();
  return (ws[slot][0] + ws[slot][1]) + (ws[slot][2] + ws[slot][3]);
}

// The value and the 3 + d derivatives from the pieces (one workgroup): thread t adds entries t, t + 256, ... in ascending
// order, then block256_sum.  sums: the d + 1 outputs of the reduction with P = K_y^-1.
__global__ __launch_bounds__(256) void gp_mll_finish_kernel(int64_t n, int d, double outputscale, const double *__restrict__ r,
                                                             const double *__restrict__ alpha, const double *__restrict__ Lc,
                                                             int64_t ldlc, const double *__restrict__ P, int64_t ldp,
                                                             const double *__restrict__ sums, double *__restrict__ out) {
  __shared__ double ws[4][4];
  double ra = 0.0, ld = 0.0, sa = 0.0, tw = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double a = alpha[i];
    ra = fma(r[i], a, ra);
    ld += log(Lc[i * ldlc + i]);
    sa += a;
    tw += __dsub_rn(__dmul_rn(a, a), P[i * ldp + i]);  // W_ii
  }
  ra = block256_sum(ra, ws, 0);
  ld = block256_sum(ld, ws, 1);
  sa = block256_sum(sa, ws, 2);
  tw = block256_sum(tw, ws, 3);
  if (threadIdx.x == 0) {
    out[0] = -0.5 * ra - ld - 0.5 * (double)n * 1.8378770664093454836;  // log 2 pi
    out[1] = sa;
    out[2] = 0.5 * tw;
    out[3] = 0.5 * outputscale * sums[0];
  }
  if ((int)threadIdx.x < d) out[4 + threadIdx.x] = 0.5 * sums[1 + threadIdx.x];
}

struct GpMllPlan {  // offsets in doubles into the workspace of pls_gp_mll_grad
  int64_t ld, plane, r, alpha, partials, sums, total;
};
static GpMllPlan gp_mll_plan(int64_t n, int64_t d) {
  GpMllPlan p;
  p.ld = gp_mll_ld(n);
  p.plane = n * p.ld;
  p.r = 7 * p.plane;
  p.alpha = p.r + gp_mll_vec(n);
  p.partials = p.alpha + gp_mll_vec(n);
  p.sums = p.partials + gp_mll_vec(grad_sums_blocks(n) * (d + 1));
  p.total = p.sums + gp_mll_vec(d + 1);
  return p;
}

static bool stationary_kind(int32_t kind) {
  return kind == PLS_KERNEL_RBF_ARD || kind == PLS_KERNEL_MATERN12 || kind == PLS_KERNEL_MATERN32 || kind == PLS_KERNEL_MATERN52;
}

// What pls_kernel_grad_sums, pls_gp_mll_grad and pls_gp_mll_grad_classes check alike, each under its own name `who`: the
// kernel kind, the sizes (classes == NULL: the entry has no class axis), the grid limit of the reduction and the
// workspace of `need` bytes on an `align`-byte boundary.  The entry's own checks follow it.
static int gp_check_shared(const char *who, int32_t kernel_kind, int64_t n, int64_t d, const int64_t *classes,
                           const void *workspace, size_t workspace_bytes, size_t need, int align) {
  PLS_REQUIRE(kernel_kind != PLS_KERNEL_LINEAR, "%s: the linear kernel has no lengthscale or outputscale to learn", who);
  PLS_REQUIRE(stationary_kind(kernel_kind), "%s: unknown kernel kind %d", who, kernel_kind);
  if (classes)
    PLS_REQUIRE(n > 0 && d > 0 && *classes > 0, "%s: bad sizes n=%lld d=%lld classes=%lld", who, (long long)n, (long long)d,
                (long long)*classes);
  PLS_REQUIRE(n > 0 && d > 0, "%s: bad sizes n=%lld d=%lld", who, (long long)n, (long long)d);
  PLS_REQUIRE(d <= GRAD_D_MAX, "%s: input dimension %lld > 64 is not supported", who, (long long)d);
  PLS_REQUIRE(cdiv(n, GRAD_ROWS) <= 65535, "%s: n=%lld too large", who, (long long)n);
  PLS_REQUIRE(workspace, "%s: NULL workspace", who);
  if (workspace_bytes < need)
    return fail(PLS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  PLS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & (uintptr_t)(align - 1)) == 0, "%s: workspace must be %d-byte aligned", who,
              align);
  return PLS_OK;
}

// out = in + diag(fixed + shift)  (m x m): the vector form of scale_add_diag_kernel (chol.hip), for a noise that differs
// from point to point
__global__ __launch_bounds__(256) void add_diag_vector_kernel(const double *__restrict__ in, int64_t ldi,
                                                               const double *__restrict__ fixed, double shift,
                                                               double *__restrict__ out, int64_t ldo, int64_t m) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= m) return;
  for (int64_t row = blockIdx.y; row < m; row += gridDim.y) {
    const double v = in[row * ldi + col];
    out[row * ldo + col] = (row == col) ? v + (fixed[row] + shift) : v;
  }
}

// One evaluation in the workspace w (arguments already validated): pls_gp_mll_grad with fixed == NULL, one class of
// pls_gp_mll_grad_classes otherwise (K_y = s kappa + diag(fixed + noise + jitter)).
static int gp_mll_evaluate(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                           double outputscale, double noise, double mean, double jitter, const double *fixed, const double *y,
                           double *out, int32_t *info, double *w, void *stream) {
  hipStream_t st = S(stream);
  const GpMllPlan p = gp_mll_plan(n, d);
  double *Ky = w, *Lc = w + p.plane, *LcT = w + 2 * p.plane, *Sf = w + 3 * p.plane, *Sb = w + 4 * p.plane;
  double *Linv = w + 5 * p.plane, *LinvT = w + 6 * p.plane;
  double *r = w + p.r, *al = w + p.alpha, *partials = w + p.partials, *sums = w + p.sums;
  // 1. K_y = s kappa(x, x) + (noise + jitter) I [+ diag(fixed)]   (the Gram matrix passes through the plane of Linv, still free)
  int rc = pls_kernel_gram(kernel_kind, x, n, x, n, d, lengthscale, outputscale, Linv, p.ld, stream);
  if (rc) return rc;
  if (fixed) {
    const unsigned gy = (unsigned)(n < 1024 ? n : 1024);
    hipLaunchKernelGGL(add_diag_vector_kernel, dim3((unsigned)cdiv(n, 256), gy), dim3(256), 0, st, Linv, p.ld, fixed,
                       noise + jitter, Ky, p.ld, n);
    rc = check_launch("add_diag_vector");
  } else {
    rc = launch_scale_add_diag(Linv, p.ld, 1.0, noise + jitter, Ky, p.ld, n, st);
  }
  if (rc) return rc;
  // 2. K_y = Lc Lc^T and the substitution operators
  rc = pls_chol_factor(Ky, p.ld, n, 0.0, Lc, p.ld, LcT, p.ld, Sf, p.ld, Sb, p.ld, info, stream);
  if (rc) return rc;
  pls_chol_desc f{};
  f.m = n;
  f.Lc = Lc, f.ldlc = p.ld, f.LcT = LcT, f.ldlct = p.ld, f.Sf = Sf, f.ldsf = p.ld, f.Sb = Sb, f.ldsb = p.ld;
  // 3. alpha = K_y^-1 (y - mean)
  hipLaunchKernelGGL(gp_center_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, y, mean, n, r);
  if ((rc = check_launch("gp_center"))) return rc;
  rc = pls_chol_solve(&f, r, 1, 1, al, 1, stream);
  if (rc) return rc;
  // 4. Linv = Lc^-1, then P = K_y^-1 = Linv^T Linv over the plane of K_y (Linv lower triangular: only k >= row contracted)
  rc = pls_chol_build_inverse(&f, Linv, p.ld, LinvT, p.ld, stream);
  if (rc) return rc;
  rc = gemm_tn_ex(Linv, p.ld, Linv, p.ld, Ky, p.ld, n, n, n, 1.0, 0.0, 2, st);
  if (rc) return rc;
  // 5. the d + 1 sums with P = K_y^-1
  rc = grad_sums_launch(kernel_kind, x, n, (int)d, lengthscale, outputscale, al, Ky, p.ld, sums, partials, st);
  if (rc) return rc;
  // 6. value and derivatives
  hipLaunchKernelGGL(gp_mll_finish_kernel, dim3(1), dim3(256), 0, st, n, (int)d, outputscale, r, al, Lc, p.ld, Ky, p.ld, sums, out);
  return check_launch("gp_mll_finish");
}

// The C >= 1 evaluations of both pls_gp_mll_grad entries, one after another in the shared workspace w (arguments already
// validated); fixed == NULL: no fixed noise
static int gp_mll_evaluate_classes(int32_t kernel_kind, const double *x, int64_t n, int64_t d, int64_t classes,
                                   const double *lengthscale, const double *outputscale, const double *noise, const double *mean,
                                   const double *fixed, int64_t ldf, const double *y, int64_t ldy, double jitter, double *out,
                                   int32_t *info, double *w, void *stream) {
  for (int64_t c = 0; c < classes; ++c) {
    const int rc = gp_mll_evaluate(kernel_kind, x, n, d, lengthscale + c * d, outputscale[c], noise[c], mean[c], jitter,
                                   fixed ? fixed + c * ldf : nullptr, y + c * ldy, out + c * (4 + d), info + c, w, stream);
    if (rc) return rc;
  }
  return PLS_OK;
}

// Class probabilities of a Dirichlet GP: out[i][c] = (1/S) sum_s softmax_c(mu[.][i] + sqrt(max(var[.][i], 0)) z[s][.]) with
// z[s][c] element (row s, column c) of the library's normal matrix for step = first_point + i under `seed` (philox.h;
// rows s and s ^ 4 share one Philox call and are handled by the same lane).
// One wave per test point.  Pair p (p = 0, 1, ...) holds the samples s = 8 (p / 4) + p % 4 and s + 4; lane l takes the pairs
// l, l + 64, ... in ascending order and adds, per class, sample s and then sample s + 4 into its accumulator (samples
// >= S are skipped); the 64 accumulators are added by an xor butterfly (offsets 32, 16, ..., 1); the total is divided by
// S.  No atomics: the order is fixed, two calls give the same bits.  The softmax subtracts the row maximum, so every
// exponent is <= 0 (exp_nonpos: exactly 0 below -745.2, exactly 1 at 0).
template <int C_MAX>
__global__ __launch_bounds__(256) void softmax_normal_mean_kernel(const double *__restrict__ mu, int64_t ldmu,
                                                                   const double *__restrict__ var, int64_t ldvar, int classes,
                                                                   int64_t t, int64_t samples, uint64_t seed, uint64_t first_point,
                                                                   double *__restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= t) return;  // (a whole wave)
  double m[C_MAX], sd[C_MAX], acc[C_MAX];
#pragma unroll
  for (int c = 0; c < C_MAX; ++c) {
    m[c] = (c < classes) ? mu[c * ldmu + i] : 0.0;
    sd[c] = (c < classes) ? sqrt(fmax(var[c * ldvar + i], 0.0)) : 0.0;
    acc[c] = 0.0;
  }
  const uint64_t step = first_point + (uint64_t)i;
  const int64_t pairs = 4 * cdiv(samples, (int64_t)8);
  for (int64_t p = lane; p < pairs; p += 64) {
    const int64_t s0 = 8 * (p >> 2) + (p & 3);
    if (s0 >= samples) continue;
    const bool two = s0 + 4 < samples;
    double a0[C_MAX], a1[C_MAX];
    double max0 = -__builtin_huge_val(), max1 = -__builtin_huge_val();
#pragma unroll
    for (int c = 0; c < C_MAX; ++c) {
      if (c < classes) {
        double z_lo, z_hi;
        normal_pair(seed, step, s0, c, z_lo, z_hi);
        a0[c] = fma(sd[c], z_lo, m[c]);
        a1[c] = fma(sd[c], z_hi, m[c]);
        max0 = fmax(max0, a0[c]);
        max1 = fmax(max1, a1[c]);
      }
    }
    double sum0 = 0.0, sum1 = 0.0;
#pragma unroll
    for (int c = 0; c < C_MAX; ++c) {
      if (c < classes) {
        a0[c] = exp_nonpos(a0[c] - max0);
        a1[c] = exp_nonpos(a1[c] - max1);
        sum0 += a0[c];
        sum1 += a1[c];
      }
    }
#pragma unroll
    for (int c = 0; c < C_MAX; ++c) {
      if (c < classes) {
        acc[c] += a0[c] / sum0;
        if (two) acc[c] += a1[c] / sum1;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C_MAX; ++c) {
    if (c < classes) {
      double v = acc[c];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) out[i * ldo + c] = v / (double)samples;
    }
  }
}

static int softmax_normal_mean_launch(const double *mu, int64_t ldmu, const double *var, int64_t ldvar, int classes, int64_t t,
                                      int64_t samples, uint64_t seed, uint64_t first_point, double *out, int64_t ldo,
                                      hipStream_t st) {
  const dim3 grid((unsigned)cdiv(t, (int64_t)4));
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
#define PLS_SOFTMAX_CASE(CM)                                                                                        \
  hipLaunchKernelGGL((softmax_normal_mean_kernel<CM>), grid, dim3(256), 0, st, mu, ldmu, var, ldvar, classes, t, samples, \
                     seed, first_point, out, ldo)
    if (classes <= 2) PLS_SOFTMAX_CASE(2);
    else if (classes <= 4) PLS_SOFTMAX_CASE(4);
    else if (classes <= 8) PLS_SOFTMAX_CASE(8);
    else if (classes <= 16) PLS_SOFTMAX_CASE(16);
    else if (classes <= 32) PLS_SOFTMAX_CASE(32);
    else PLS_SOFTMAX_CASE(64);
#undef PLS_SOFTMAX_CASE
  }
  return check_launch("softmax_normal_mean");
}
}  // namespace plship

using namespace plship;

extern "C" {

size_t pls_kernel_grad_sums_workspace_bytes(int64_t n, int64_t d) {
  return (n > 0 && d > 0 && d <= GRAD_D_MAX) ? grad_sums_workspace_bytes(n, d) : 0;
}

int pls_kernel_grad_sums(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                         double outputscale, const double *alpha, const double *P, int64_t ldp, double *out, void *workspace,
                         size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("kernel_grad_sums", kernel_kind, n, d, nullptr, workspace, workspace_bytes,
                               pls_kernel_grad_sums_workspace_bytes(n, d), 8))
    return rc;
  PLS_REQUIRE(x && lengthscale && alpha && P && out, "kernel_grad_sums: NULL pointer");
  PLS_REQUIRE(ldp >= n, "kernel_grad_sums: ldp < n");
  return grad_sums_launch(kernel_kind, x, n, (int)d, lengthscale, outputscale, alpha, P, ldp, out,
                          static_cast<double *>(workspace), S(stream));
}

int pls_kernel_mean(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale, double outputscale,
                    double mean, const double *alpha, const double *xt, int64_t t, double *out, void *stream) {
  PLS_REQUIRE(kernel_kind != PLS_KERNEL_LINEAR, "kernel_mean: the linear kernel has no lengthscale or outputscale to learn");
  PLS_REQUIRE(stationary_kind(kernel_kind), "kernel_mean: unknown kernel kind %d", kernel_kind);
  PLS_REQUIRE(n > 0 && d > 0 && t >= 0, "kernel_mean: bad sizes n=%lld d=%lld t=%lld", (long long)n, (long long)d, (long long)t);
  PLS_REQUIRE(d <= GRAD_D_MAX, "kernel_mean: input dimension %lld > 64 is not supported", (long long)d);
  PLS_REQUIRE(cdiv(t, (int64_t)MEAN_POINTS) <= 2147483647, "kernel_mean: t=%lld too large", (long long)t);
  if (t == 0) return PLS_OK;
  PLS_REQUIRE(x && lengthscale && alpha && xt && out, "kernel_mean: NULL pointer");
  return kernel_mean_launch(kernel_kind, x, n, (int)d, lengthscale, outputscale, mean, alpha, xt, t, out, S(stream));
}

size_t pls_gp_mll_workspace_bytes(int64_t n, int64_t d) {
  return (n > 0 && d > 0 && d <= GRAD_D_MAX) ? (size_t)gp_mll_plan(n, d).total * sizeof(double) : 0;
}

// pls_gp_mll_grad_classes with one class and no fixed noise: the scalars go in as arrays of one
int pls_gp_mll_grad(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale, double outputscale,
                    double noise, double mean, double jitter, const double *y, double *out, int32_t *info, void *workspace,
                    size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("gp_mll_grad", kernel_kind, n, d, nullptr, workspace, workspace_bytes,
                               pls_gp_mll_workspace_bytes(n, d), 16))
    return rc;
  PLS_REQUIRE(x && lengthscale && y && out && info, "gp_mll_grad: NULL pointer");
  PLS_REQUIRE(jitter >= 0.0, "gp_mll_grad: jitter must be >= 0");
  PLS_REQUIRE(noise >= 0.0, "gp_mll_grad: noise must be >= 0");
  return gp_mll_evaluate_classes(kernel_kind, x, n, d, 1, lengthscale, &outputscale, &noise, &mean, nullptr, n, y, n, jitter, out,
                                 info, static_cast<double *>(workspace), stream);
}

size_t pls_gp_mll_classes_workspace_bytes(int64_t n, int64_t d, int64_t classes) {
  return classes > 0 ? pls_gp_mll_workspace_bytes(n, d) : 0;  // the classes run one after another and share the planes
}

int pls_gp_mll_grad_classes(int32_t kernel_kind, const double *x, int64_t n, int64_t d, int64_t classes,
                            const double *lengthscale, const double *outputscale, const double *noise, const double *mean,
                            const double *fixed_noise, int64_t ldf, const double *y, int64_t ldy, double jitter, double *out,
                            int32_t *info, void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("gp_mll_grad_classes", kernel_kind, n, d, &classes, workspace, workspace_bytes,
                               pls_gp_mll_classes_workspace_bytes(n, d, classes), 16))
    return rc;
  PLS_REQUIRE(x && lengthscale && outputscale && noise && mean && y && out && info, "gp_mll_grad_classes: NULL pointer");
  PLS_REQUIRE(ldy >= n, "gp_mll_grad_classes: ldy < n");
  PLS_REQUIRE(!fixed_noise || ldf >= n, "gp_mll_grad_classes: ldf < n");
  PLS_REQUIRE(jitter >= 0.0, "gp_mll_grad_classes: jitter must be >= 0");
  for (int64_t c = 0; c < classes; ++c)  // (host arrays: read only after the pointer checks)
    PLS_REQUIRE(noise[c] >= 0.0, "gp_mll_grad_classes: noise must be >= 0 (class %lld)", (long long)c);
  return gp_mll_evaluate_classes(kernel_kind, x, n, d, classes, lengthscale, outputscale, noise, mean, fixed_noise, ldf, y, ldy,
                                 jitter, out, info, static_cast<double *>(workspace), stream);
}

int pls_softmax_normal_mean(const double *mu, int64_t ldmu, const double *var, int64_t ldvar, int64_t classes, int64_t t,
                            int64_t samples, uint64_t seed, uint64_t first_point, double *out, int64_t ldo, void *stream) {
  PLS_REQUIRE(classes > 0 && t > 0 && samples > 0, "softmax_normal_mean: bad sizes classes=%lld t=%lld samples=%lld",
              (long long)classes, (long long)t, (long long)samples);
  PLS_REQUIRE(classes <= 64, "softmax_normal_mean: %lld classes > 64 are not supported", (long long)classes);
  PLS_REQUIRE(cdiv(t, (int64_t)4) <= 2147483647, "softmax_normal_mean: t=%lld too large", (long long)t);
  PLS_REQUIRE(mu && var && out, "softmax_normal_mean: NULL pointer");
  PLS_REQUIRE(ldmu >= t && ldvar >= t, "softmax_normal_mean: ldmu / ldvar < t");
  PLS_REQUIRE(ldo >= classes, "softmax_normal_mean: ldo < classes");
  return softmax_normal_mean_launch(mu, ldmu, var, ldvar, (int)classes, t, samples, seed, first_point, out, ldo, S(stream));
}

}  // extern "C"
