// Exact-GP marginal log-likelihood and its gradient with respect to the base-kernel hyper-parameters.
//
// Reference: mll(model(x), y) and loss.backward() of train_exact_gp (experiments/trainers.py:45-49), i.e. gpytorch's
// ExactMarginalLogLikelihood of ScaleKernel(RBFKernel | MaternKernel | RQKernel) + GaussianLikelihood with a constant mean.
//
//   K_y = s kappa(x, x) + (noise + jitter) I = Lc Lc^T,   r = y - mean,   alpha = K_y^-1 r,   W = alpha alpha^T - K_y^-1
//   mll = -1/2 r^T alpha - sum_i log Lc_ii - n/2 log 2 pi,                d mll / d theta = 1/2 sum_ij W_ij dK_ij / d theta
//
// The Gram build, the factorisation, the solve, the inverse factor and K_y^-1 = Linv^T Linv are the library's existing
// kernels; the reduction over all n^2 pairs is kernel_grad_sums_kernel (base_kernel.hip): one pass over P (= K_y^-1) that
// recomputes kappa and its lengthscale derivatives from x and leaves the d + 1 sums sum_ij W_ij kappa_ij and
// sum_ij W_ij dK_ij / d log l_k in a fixed summation order (RQ: d + 2, the last is sum_ij W_ij dK_ij / d log alpha).
//
// Classification (gpytorch's DirichletClassificationLikelihood, Milios et al. 2018): one such GP per class on the shared
// x, K_y,c = s_c kappa(x, x; l_c) + diag(v_c) + sigma_c I with a fixed noise v_c per point -- pls_gp_mll_grad_classes runs
// the same evaluation per class with the diagonal as a vector (add_diag_vector_kernel); softmax_normal_mean_kernel turns
// the latent means and variances at test points into class probabilities on the library's Philox stream.
#include <hip/hip_runtime.h>

#define PLS_SCALAR_POLY_CONSTANTS 1  // (fmath.h: the exp polynomial's constants as scalar operands, as in the Gram build)
#include "../../include/plship.h"
#include "base_kernel.h"
#include "chol.h"
#include "common.h"
#include "gemm_api.h"
#include "gp_mll.h"
#include "kernel_math.h"
#include "philox.h"

namespace plship {

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
// order, then block256_sum.  sums: the nsums outputs of the reduction with P = K_y^-1 (d + 1; RQ: d + 2, whose last becomes
// the derivative with respect to log alpha, out[4 + d]; trend plus seasonal: 4 d + 2, sums[0] the trend's kappa sum, so out[3]
// is the derivative with respect to log s_t, and the last the one with respect to log s_s, out[4 + 4 d]).
__global__ __launch_bounds__(256) void gp_mll_finish_kernel(int64_t n, int nsums, double outputscale, const double *__restrict__ r,
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
  if ((int)threadIdx.x < nsums - 1) out[4 + threadIdx.x] = 0.5 * sums[1 + threadIdx.x];
}

struct GpMllPlan {  // offsets in doubles into the workspace of pls_gp_mll_grad
  int64_t ld, plane, r, alpha, partials, sums, total;
};
static GpMllPlan gp_mll_plan(int32_t kind, int64_t n, int64_t d) {
  GpMllPlan p;
  p.ld = gp_mll_ld(n);
  p.plane = n * p.ld;
  p.r = 7 * p.plane;
  p.alpha = p.r + gp_mll_vec(n);
  p.partials = p.alpha + gp_mll_vec(n);
  p.sums = p.partials + gp_mll_vec(grad_sums_blocks(n) * grad_sums_count(kind, d));
  p.total = p.sums + gp_mll_vec(grad_sums_count(kind, d));
  return p;
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
  const GpMllPlan p = gp_mll_plan(kernel_kind, n, d);
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
  // 5. the d + 1 sums (RQ: d + 2; periodic: 2 d + 1; locally periodic: 3 d + 1; trend plus seasonal: 4 d + 2) with P = K_y^-1
  rc = grad_sums_launch(kernel_kind, x, n, (int)d, lengthscale, outputscale, al, Ky, p.ld, sums, partials, st);
  if (rc) return rc;
  // 6. value and derivatives
  hipLaunchKernelGGL(gp_mll_finish_kernel, dim3(1), dim3(256), 0, st, n, (int)grad_sums_count(kernel_kind, d), outputscale, r,
                     al, Lc, p.ld, Ky, p.ld, sums, out);
  return check_launch("gp_mll_finish");
}

// The C >= 1 evaluations of both pls_gp_mll_grad entries, one after another in the shared workspace w (arguments already
// validated); fixed == NULL: no fixed noise.  A class's row of `lengthscale` holds its shape parameters behind its d
// lengthscales, its row of `out` their derivatives behind the d lengthscale derivatives.
static int gp_mll_evaluate_classes(int32_t kernel_kind, const double *x, int64_t n, int64_t d, int64_t classes,
                                   const double *lengthscale, const double *outputscale, const double *noise, const double *mean,
                                   const double *fixed, int64_t ldf, const double *y, int64_t ldy, double jitter, double *out,
                                   int32_t *info, double *w, void *stream) {
  const int64_t extra = kind_shape_params(kernel_kind, d);
  for (int64_t c = 0; c < classes; ++c) {
    const int rc = gp_mll_evaluate(kernel_kind, x, n, d, lengthscale + c * (d + extra), outputscale[c], noise[c], mean[c], jitter,
                                   fixed ? fixed + c * ldf : nullptr, y + c * ldy, out + c * (4 + d + extra), info + c, w, stream);
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

size_t pls_gp_mll_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d) {
  return (stationary_kind(kernel_kind) && n > 0 && d > 0 && d <= kind_d_max(kernel_kind))
             ? (size_t)gp_mll_plan(kernel_kind, n, d).total * sizeof(double)
             : 0;
}
size_t pls_gp_mll_workspace_bytes(int64_t n, int64_t d) { return pls_gp_mll_workspace_bytes_kind(PLS_KERNEL_RBF_ARD, n, d); }

// pls_gp_mll_grad_classes with one class and no fixed noise: the scalars go in as arrays of one
int pls_gp_mll_grad(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale, double outputscale,
                    double noise, double mean, double jitter, const double *y, double *out, int32_t *info, void *workspace,
                    size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("gp_mll_grad", kernel_kind, n, d, nullptr, workspace, workspace_bytes,
                               pls_gp_mll_workspace_bytes_kind(kernel_kind, n, d), 16))
    return rc;
  PLS_REQUIRE(x && lengthscale && y && out && info, "gp_mll_grad: NULL pointer");
  PLS_REQUIRE(jitter >= 0.0, "gp_mll_grad: jitter must be >= 0");
  PLS_REQUIRE(noise >= 0.0, "gp_mll_grad: noise must be >= 0");
  return gp_mll_evaluate_classes(kernel_kind, x, n, d, 1, lengthscale, &outputscale, &noise, &mean, nullptr, n, y, n, jitter, out,
                                 info, static_cast<double *>(workspace), stream);
}

size_t pls_gp_mll_classes_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d, int64_t classes) {
  return classes > 0 ? pls_gp_mll_workspace_bytes_kind(kernel_kind, n, d) : 0;  // the classes run one after another and share the planes
}
size_t pls_gp_mll_classes_workspace_bytes(int64_t n, int64_t d, int64_t classes) {
  return pls_gp_mll_classes_workspace_bytes_kind(PLS_KERNEL_RBF_ARD, n, d, classes);
}

int pls_gp_mll_grad_classes(int32_t kernel_kind, const double *x, int64_t n, int64_t d, int64_t classes,
                            const double *lengthscale, const double *outputscale, const double *noise, const double *mean,
                            const double *fixed_noise, int64_t ldf, const double *y, int64_t ldy, double jitter, double *out,
                            int32_t *info, void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("gp_mll_grad_classes", kernel_kind, n, d, &classes, workspace, workspace_bytes,
                               pls_gp_mll_classes_workspace_bytes_kind(kernel_kind, n, d, classes), 16))
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
