// Sparse variational GP with a FIXED kernel and FIXED inducing points: the minibatch ELBO, its gradient, the SGD epoch and
// the prediction, with a Gaussian likelihood (closed form) or a Bernoulli / Student-t likelihood (20-node Gauss-Hermite).
//
// Reference: SVGP (src/gaussian_process/svgp.py:6-49), train_svgp with is_fixed=True (experiments/trainers.py:55-136) and
// train_svgp_for_profiler (experiments/profiler/main.py:85-123).  The arithmetic is gpytorch 1.15's whitened
// VariationalStrategy + CholeskyVariationalDistribution + VariationalELBO + GaussianLikelihood AS RECALLED (gpytorch is
// not available to this project); the formulas in include/plship.h are the contract.
//
// With At (n x M) the rows a_i of (L^-1 k(Z, X))^T, q_i the whitened residual variance and the state m, L_s, c, rho:
//   mu_i = c + a_i . m      w_i = L_s^T a_i      v_i = q_i + |w_i|^2      sigma^2 = softplus(rho) + 1e-4
//
// Two launches per evaluation, no atomics, every sum in a fixed order:
//   svgp_batch_kernel   one workgroup (4 waves) per tile of SVGP_TILE = 32 points.  The tile's rows of At are gathered by
//                       index into LDS (zero padded to MP = M rounded up to 16).  w = a L_s runs on v_mfma_f64_16x16x4:
//                       wave v owns the 16-column tiles v, v + 4, ... of w for both 16-point row tiles; L_s is streamed
//                       in 4-row k-panels straight from memory into the B fragment (an element of L_s is used by one wave
//                       of a workgroup only, so an LDS copy would be written and read once), rows above the column's
//                       diagonal are skipped and the upper triangle is never read.  Then mu and |w|^2 (a wave per point:
//                       lane l adds k = l, l + 64, ...; xor butterfly 32 ... 1), the per-point likelihood epilogue (the
//                       Gaussian one on lane 0; the quadrature ones after the wave's 8 points are known: 8 lanes per
//                       point, lane s of a group adds nodes s, s + 8, s + 16 in that order, xor butterfly 4, 2, 1), the
//                       tile's three scalar sums (xor butterfly over its 32 points), sum_i g_mu,i a_i (thread k adds the
//                       points in ascending order) and the tile's partial of sum_i g_v,i a_i w_i^T: the lower 16 x 16
//                       tiles dealt to the waves round-robin, 8 MFMAs each with the accumulator in place.  Workgroup 0
//                       also leaves the three KL sums of the state it read.
//   svgp_finish_kernel  workgroup k < M: row k of grad L_s -- thread l <= k adds the tiles' partials in ascending tile
//                       order, then the KL term;  the last workgroup: grad m likewise and the scalars (thread t adds tiles
//                       t, t + 256, ...; butterfly; (w0 + w1) + (w2 + w3)).  In update mode the same threads apply
//                       p <- p - lr * (-g) as a multiply and a subtract (no contraction), so a replay of
//                       pls_svgp_elbo_grad + the same two operations elsewhere gives the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/plship.h"
#include "common.h"
#include "svgp.h"

namespace plship {

typedef double svgp_d4 __attribute__((ext_vector_type(4)));

// No contraction in this unit: a multiply followed by an add or a subtract stays two roundings (the SGD update must equal
// its replay elsewhere bit for bit); where a fused multiply-add is wanted it is written as fma().  The pragma covers the
// operators written HERE: the __dmul_rn / __dsub_rn wrappers of the HIP headers are inlined with the header's own setting
// and do get fused, so the update below uses plain operators.
#pragma clang fp contract(off)

constexpr double SVGP_MIN_NOISE = 1e-4;                   // gpytorch's GreaterThan(1e-4) on the likelihood noise
constexpr double SVGP_HALF_LOG_2PI = 0.91893853320467274178;

__device__ __forceinline__ double svgp_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double svgp_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

__device__ __forceinline__ double svgp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum_k x[k] y[k], k < mp: lane l adds k = l, l + 64, ... in ascending order, then the butterfly; every lane returns it
__device__ __forceinline__ double svgp_wave_dot(const double *x, const double *y, int mp) {
  double s = 0.0;
  for (int k = threadIdx.x & 63; k < mp; k += 64) s = fma(x[k], y[k], s);
  return svgp_wave_sum(s);
}

// workgroup sum of one value per thread: butterfly inside each wave, then (w0 + w1) + (w2 + w3); red: 4 doubles of LDS
__device__ __forceinline__ double svgp_block_sum(double v, double *red) {
  v = svgp_wave_sum(v);
  __syncthreads();  // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The per-point likelihood epilogue: from y, mu, v and sigma^2 the expected log-likelihood ell, g_mu = d ell / d mu,
// g_v = d ell / d v and d ell / d sigma^2.  The contractions around it do not know the likelihood.
template <int LIK>
struct SvgpEpilogue;
template <>
struct SvgpEpilogue<PLS_SVGP_GAUSSIAN> {
  __device__ __forceinline__ static void eval(double y, double mu, double v, double sig2, double &ell, double &gmu, double &gv,
                                              double &dsig2) {
    const double r = y - mu;
    const double e = fma(r, r, v);
    const double h = 0.5 / sig2;
    ell = -SVGP_HALF_LOG_2PI - 0.5 * log(sig2) - e * h;
    gmu = r / sig2;
    gv = -h;
    dsig2 = -h + e * h / sig2;
  }
};

// The quadrature likelihoods (include/plship.h, "SVGP with a quadrature likelihood"): l = sum_k w^_k g(f_k) over the
// SVGP_Q Gauss-Hermite nodes f_k = mu + sqrt(2 v) x_k, with g_mu and g_v the derivatives of that SUM.  x_k, omega_k are
// numpy.polynomial.hermite.hermgauss(20) as doubles; w^_k = omega_k / sqrt(pi) rounded once.
constexpr int SVGP_Q = 20;
__constant__ double svgp_gh_x[SVGP_Q] = {
    -5.3874808900112328,  -4.6036824495507442,  -3.9447640401156252,  -3.3478545673832163, -2.7888060584281305,
    -2.2549740020892757,  -1.7385377121165861,  -1.2340762153953231,  -0.73747372854539439, -0.24534070830090124,
    0.24534070830090124,  0.73747372854539439,  1.2340762153953231,   1.7385377121165861,  2.2549740020892757,
    2.7888060584281305,   3.3478545673832163,   3.9447640401156252,   4.6036824495507442,  5.3874808900112328};
__constant__ double svgp_gh_w[SVGP_Q] = {
    1.2578006724379234e-13, 2.4820623623151755e-10, 6.127490259982928e-08, 4.402121090230851e-06, 0.00012882627996192928,
    0.0018301031310804898,  0.013997837447101022,   0.06150637206397689,   0.16173933398399998,   0.26079306344955483,
    0.26079306344955483,    0.16173933398399998,    0.06150637206397689,   0.013997837447101022,  0.0018301031310804898,
    0.00012882627996192928, 4.402121090230851e-06,  6.127490259982928e-08, 2.4820623623151755e-10, 1.2578006724379234e-13};

constexpr double SVGP_INV_SQRT2 = 0.70710678118654752440;
constexpr double SVGP_SQRT_2_OVER_PI = 0.79788456080286535588;
constexpr double SVGP_INV_SQRT_2PI = 0.39894228040143267794;

// what the likelihood adds to the arguments: Student-t's fixed degrees of freedom and the part of its log-normaliser that
// does not depend on the scale, lgamma((nu + 1) / 2) - lgamma(nu / 2) - 1/2 log(nu pi), evaluated once on the host
struct SvgpLikArgs {
  double nu, lgc;
};

// the likelihood's noise from the raw value: Gaussian softplus + 1e-4 (GreaterThan(1e-4)), Student-t softplus alone
// (Positive), Bernoulli none
template <int LIK>
__device__ __forceinline__ double svgp_noise(double rho) {
  if (LIK == PLS_SVGP_GAUSSIAN) return svgp_softplus(rho) + SVGP_MIN_NOISE;
  if (LIK == PLS_SVGP_STUDENT_T) return svgp_softplus(rho);
  return 0.0;
}

// One node: g(f), g'(f) and dg / d sigma^2.
template <int LIK>
struct SvgpNode;
// probit: g = log Phi(s f), s = 2 y - 1.  Below 0 through erfcx (Phi itself underflows from s f = -38 on), above through
// log1p of the upper tail.
template <>
struct SvgpNode<PLS_SVGP_BERNOULLI> {
  __device__ __forceinline__ static void eval(double y, double f, double, const SvgpLikArgs &, double &g, double &gp, double &gs) {
    const double s = 2.0 * y - 1.0, z = s * f;
    double ratio;
    if (z < 0.0) {
      const double t = erfcx(-z * SVGP_INV_SQRT2);
      g = log(0.5 * t) - 0.5 * (z * z);
      ratio = SVGP_SQRT_2_OVER_PI / t;
    } else {
      const double up = 0.5 * erfc(z * SVGP_INV_SQRT2);
      g = log1p(-up);
      ratio = SVGP_INV_SQRT_2PI * exp(-0.5 * (z * z)) / (1.0 - up);
    }
    gp = s * ratio;
    gs = 0.0;
  }
};
// Student-t with scale^2 = sig2 and fixed nu
template <>
struct SvgpNode<PLS_SVGP_STUDENT_T> {
  __device__ __forceinline__ static void eval(double y, double f, double sig2, const SvgpLikArgs &k, double &g, double &gp,
                                              double &gs) {
    const double r = y - f, r2 = r * r, a = k.nu * sig2, d = a + r2, np1 = k.nu + 1.0;
    g = (k.lgc - 0.5 * log(sig2)) - 0.5 * np1 * log1p(r2 / a);
    gp = np1 * r / d;
    gs = -0.5 / sig2 + np1 * r2 / (2.0 * sig2 * d);
  }
};

// The quadrature of the wave's 8 points: lane = 8 * (point of the wave) + s; lane s of a group adds its nodes s, s + 8,
// s + 16 (< SVGP_Q) in ascending order, then the group's xor butterfly 4, 2, 1 (a dead point's lanes carry zeros).  Every
// lane of a group returns the point's sums.
template <int LIK>
__device__ __forceinline__ void svgp_quadrature(bool live, double y, double mu, double v, double sig2, const SvgpLikArgs &k,
                                                double &ell, double &gmu, double &gv, double &ds) {
  const int sub = threadIdx.x & 7;
  const double sq = sqrt(2.0 * v);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (live) {
#pragma unroll
    for (int node = sub; node < SVGP_Q; node += 8) {
      const double x = svgp_gh_x[node], w = svgp_gh_w[node];
      double g, gp, gs;
      SvgpNode<LIK>::eval(y, fma(sq, x, mu), sig2, k, g, gp, gs);
      s0 = fma(w, g, s0);
      s1 = fma(w, gp, s1);
      s2 = fma(w * x, gp, s2);
      s3 = fma(w, gs, s3);
    }
  }
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
    s3 += __shfl_xor(s3, o);
  }
  ell = s0, gmu = s1, gv = live ? s2 / sq : 0.0, ds = s3;
}

// rows i0 ... i0 + np - 1 of the batch into a_s (SVGP_TILE x lda, zero beyond np and beyond column m).  A live row whose
// index lies outside 0 ... n - 1 is not read: it becomes NaN and shows in every output.
__device__ __forceinline__ void svgp_gather(const double *__restrict__ At, int64_t ldat, const int64_t *__restrict__ idx, int64_t n,
                                            int64_t i0, int np, int m, int mp, int lda, double *a_s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < SVGP_TILE; r += 4) {
    const bool live = r < np;
    int64_t src = 0;
    if (live) src = idx ? idx[i0 + r] : i0 + r;
    const bool ok = live && src >= 0 && src < n;
    for (int c = lane; c < mp; c += 64) {
      double v = 0.0;
      if (c < m && live) v = ok ? At[src * ldat + c] : __builtin_nan("");
      a_s[r * lda + c] = v;
    }
  }
}

// w_s = a_s tril(L_s)  (SVGP_TILE x mp): wave v takes the column tiles v, v + 4, ...; contraction rows below the tile's
// first column are skipped, entries above the diagonal and beyond m are taken as 0 without being read
__device__ __forceinline__ void svgp_tile_w(const double *__restrict__ Ls, int64_t ldls, int m, int mp, int lda, const double *a_s,
                                            double *w_s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const int mt = mp >> 4;
  for (int lt = wave; lt < mt; lt += 4) {
    svgp_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int col = 16 * lt + lr;
    for (int p0 = 16 * lt; p0 < mp; p0 += 4) {
      const int p = p0 + lq;
      const double b = (p >= col && p < m) ? Ls[(int64_t)p * ldls + col] : 0.0;
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_s[lr * lda + p], b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_s[(16 + lr) * lda + p], b, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      w_s[(lq + 4 * r) * lda + col] = acc0[r];
      w_s[(16 + lq + 4 * r) * lda + col] = acc1[r];
    }
  }
}

struct SvgpBatchArgs {
  const double *At;
  int64_t ldat;
  const double *q, *y;
  int64_t n;
  int m, mp;
  const double *mean, *Ls;
  int64_t ldls;
  const double *scalars;  // c, rho
  const int64_t *idx;
  int64_t b;
  double *kl, *scal, *pm, *pG;  // workspace pieces
  SvgpLikArgs lik;              // (read by the quadrature likelihoods only)
};

template <int LIK, bool GRAD>
__global__ __launch_bounds__(256) void svgp_batch_kernel(SvgpBatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double svgp_lds[];
  const int m = a.m, mp = a.mp, lda = mp + SVGP_LDS_PAD;
  double *a_s = svgp_lds, *w_s = a_s + SVGP_TILE * lda, *m_s = w_s + SVGP_TILE * lda;
  double *y_s = m_s + mp, *q_s = y_s + SVGP_TILE, *ell_s = q_s + SVGP_TILE, *gmu_s = ell_s + SVGP_TILE;
  double *gv_s = gmu_s + SVGP_TILE, *ds_s = gv_s + SVGP_TILE, *red = ds_s + SVGP_TILE;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t tile = blockIdx.x, i0 = tile * SVGP_TILE;
  const int np = (int)((a.b - i0 < SVGP_TILE) ? (a.b - i0) : SVGP_TILE);
  const double c = a.scalars[0], rho = a.scalars[1];
  const double sig2 = svgp_noise<LIK>(rho);

  svgp_gather(a.At, a.ldat, a.idx, a.n, i0, np, m, mp, lda, a_s);
  for (int k = t; k < mp; k += 256) m_s[k] = (k < m) ? a.mean[k] : 0.0;
  if (t < SVGP_TILE) {
    double yv = 0.0, qv = 0.0;
    if (t < np) {
      const int64_t src = a.idx ? a.idx[i0 + t] : i0 + t;
      if (src >= 0 && src < a.n) yv = a.y[src], qv = a.q[src];
    }
    y_s[t] = yv, q_s[t] = qv;
  }
  __syncthreads();
  svgp_tile_w(a.Ls, a.ldls, m, mp, lda, a_s, w_s);
  __syncthreads();
  // per point: mu, |w|^2 and the likelihood epilogue (a wave per point, 8 points per wave)
  if constexpr (LIK == PLS_SVGP_GAUSSIAN) {
    for (int j = 0; j < SVGP_TILE / 4; ++j) {
      const int r = wave * (SVGP_TILE / 4) + j;
      const double mu = c + svgp_wave_dot(a_s + r * lda, m_s, mp);
      const double wn = svgp_wave_dot(w_s + r * lda, w_s + r * lda, mp);
      if (lane == 0) {
        double ell = 0.0, gmu = 0.0, gv = 0.0, ds = 0.0;
        if (r < np) SvgpEpilogue<LIK>::eval(y_s[r], mu, q_s[r] + wn, sig2, ell, gmu, gv, ds);
        ell_s[r] = ell, gmu_s[r] = gmu, gv_s[r] = gv, ds_s[r] = ds;
      }
    }
  } else {
    // mu and v of the wave's 8 points are deposited first (in ell_s / gmu_s), then the 8 x SVGP_Q (point, node) pairs are
    // dealt over the 64 lanes
    for (int j = 0; j < SVGP_TILE / 4; ++j) {
      const int r = wave * (SVGP_TILE / 4) + j;
      const double mu = c + svgp_wave_dot(a_s + r * lda, m_s, mp);
      const double wn = svgp_wave_dot(w_s + r * lda, w_s + r * lda, mp);
      if (lane == 0) ell_s[r] = mu, gmu_s[r] = q_s[r] + wn;
    }
    __syncthreads();
    const int r = wave * (SVGP_TILE / 4) + (lane >> 3);
    const double mu = ell_s[r], v = gmu_s[r];
    double ell, gmu, gv, ds;
    svgp_quadrature<LIK>(r < np, y_s[r], mu, v, sig2, a.lik, ell, gmu, gv, ds);
    __syncthreads();  // (every lane holds its point's mu and v before they are overwritten)
    if ((lane & 7) == 0) ell_s[r] = ell, gmu_s[r] = gmu, gv_s[r] = gv, ds_s[r] = ds;
  }
  __syncthreads();
  if (wave == 0) {  // the tile's scalar sums: lanes 32 ... 63 carry zeros
    const bool in = lane < SVGP_TILE;
    const double s0 = svgp_wave_sum(in ? ell_s[lane] : 0.0);
    const double s1 = svgp_wave_sum(in ? gmu_s[lane] : 0.0);
    const double s2 = svgp_wave_sum(in ? ds_s[lane] : 0.0);
    if (lane == 0) {
      a.scal[4 * tile + 0] = s0, a.scal[4 * tile + 1] = s1, a.scal[4 * tile + 2] = s2, a.scal[4 * tile + 3] = 0.0;
    }
  }
  if (GRAD) {
    // sum_i g_mu,i a_i: thread k adds the tile's points in ascending order
    for (int k = t; k < mp; k += 256) {
      double s = 0.0;
#pragma unroll 8
      for (int r = 0; r < SVGP_TILE; ++r) s = fma(gmu_s[r], a_s[r * lda + k], s);
      a.pm[tile * mp + k] = s;
    }
    // the tile's partial of sum_i g_v,i a_i w_i^T: lower 16 x 16 tiles (kt >= lt), dealt to the waves round-robin
    const int lr = lane & 15, lq = lane >> 4, mt = mp >> 4;
    double *pg = a.pG + (size_t)tile * (size_t)mp * (size_t)mp;
    int j = 0;
    for (int kt = 0; kt < mt; ++kt) {
      for (int lt = 0; lt <= kt; ++lt, ++j) {
        if ((j & 3) != wave) continue;
        svgp_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int qd = 0; qd < SVGP_TILE / 4; ++qd) {
          const int i = 4 * qd + lq;
          const double av = gv_s[i] * a_s[i * lda + 16 * kt + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, w_s[i * lda + 16 * lt + lr], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pg[(size_t)(16 * kt + lq + 4 * r) * mp + 16 * lt + lr] = acc[r];
      }
    }
  }
  if (blockIdx.x == 0) {
    // the KL sums of the state: |tril L_s|_F^2 (thread l adds column l downwards), |m|^2, sum_p log |L_s,pp|
    double s2 = 0.0, m2 = 0.0, lg = 0.0;
    if (t < m) {
      for (int k = t; k < m; ++k) {
        const double v = a.Ls[(int64_t)k * a.ldls + t];
        s2 = fma(v, v, s2);
      }
      m2 = m_s[t] * m_s[t];
      lg = log(fabs(a.Ls[(int64_t)t * a.ldls + t]));
    }
    s2 = svgp_block_sum(s2, red);
    m2 = svgp_block_sum(m2, red);
    lg = svgp_block_sum(lg, red);
    if (t == 0) a.kl[0] = s2, a.kl[1] = m2, a.kl[2] = lg, a.kl[3] = 0.0;
  }
}

struct SvgpFinishArgs {
  int m, mp, rows;  // rows: m with gradients (one workgroup per row of grad L_s), 0 value-only
  int64_t n, b, tiles;
  const double *kl, *scal, *pm, *pG;
  double *mean, *Ls;
  int64_t ldls;
  double *scalars;
  double *out, *grad_m, *grad_L;
  int64_t ldgl;
  int update, flags, lik;  // lik: Bernoulli has no likelihood parameter -- d/drho = 0 exactly and rho is never written
  double lr;
  double *loss_out;
};

__global__ __launch_bounds__(256) void svgp_finish_kernel(SvgpFinishArgs a) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const double bd = (double)a.b, nd = (double)a.n;
  if ((int)blockIdx.x < a.rows) {
    const int k = blockIdx.x, l = t;
    if (l > k) return;
    const double *p = a.pG + (size_t)k * a.mp + l;
    const size_t plane = (size_t)a.mp * (size_t)a.mp;
    double s = 0.0;
    for (int64_t tile = 0; tile < a.tiles; ++tile) s += p[tile * plane];
    const double lv = a.Ls[(int64_t)k * a.ldls + l];
    const double pen = (l == k) ? lv - 1.0 / lv : lv;
    const double g = (2.0 * s) / bd - pen / nd;
    if (a.grad_L) a.grad_L[(int64_t)k * a.ldgl + l] = g;
    if (a.update) a.Ls[(int64_t)k * a.ldls + l] = lv - a.lr * (-g);  // (two roundings: contraction is off in this unit)
    return;
  }
  if (a.rows && t < a.m) {
    double s = 0.0;
    for (int64_t tile = 0; tile < a.tiles; ++tile) s += a.pm[tile * a.mp + t];
    const double mv = a.mean[t];
    const double g = s / bd - mv / nd;
    if (a.grad_m) a.grad_m[t] = g;
    if (a.update) a.mean[t] = mv - a.lr * (-g);
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t tile = t; tile < a.tiles; tile += 256) {
    s0 += a.scal[4 * tile + 0];
    s1 += a.scal[4 * tile + 1];
    s2 += a.scal[4 * tile + 2];
  }
  s0 = svgp_block_sum(s0, red);
  s1 = svgp_block_sum(s1, red);
  s2 = svgp_block_sum(s2, red);
  if (t == 0) {
    const double c = a.scalars[0], rho = a.scalars[1];
    const double ell = s0 / bd;
    const double kl = 0.5 * (((a.kl[0] + a.kl[1]) - (double)a.m) - 2.0 * a.kl[2]);
    const double elbo = ell - kl / nd;
    const double gc = s1 / bd;
    const bool has_noise = a.lik != PLS_SVGP_BERNOULLI;
    const double grho = has_noise ? svgp_sigmoid(rho) * (s2 / bd) : 0.0;
    if (a.out) a.out[0] = elbo, a.out[1] = gc, a.out[2] = grho, a.out[3] = ell, a.out[4] = kl;
    if (a.loss_out) a.loss_out[0] = -elbo;
    if (a.update) {
      if (a.flags & PLS_SVGP_TRAIN_MEAN) a.scalars[0] = c - a.lr * (-gc);
      if ((a.flags & PLS_SVGP_TRAIN_NOISE) && has_noise) a.scalars[1] = rho - a.lr * (-grho);
    }
  }
}

// mean and latent variance at t points (no sums across points) and, where obs_out is given, the likelihood's variance of
// an observation there: Gaussian v + sigma^2, Student-t v + sigma^2 nu / (nu - 2), Bernoulli p (1 - p) at
// p = Phi(mu / sqrt(1 + v)) with 1 - p taken as Phi(-...)
template <int LIK>
__global__ __launch_bounds__(256) void svgp_predict_kernel(const double *__restrict__ At, int64_t ldat, const double *__restrict__ q,
                                                            int64_t tn, int m, int mp, const double *__restrict__ mean,
                                                            const double *__restrict__ Ls, int64_t ldls,
                                                            const double *__restrict__ scalars, double *__restrict__ mean_out,
                                                            double *__restrict__ var_out, double *__restrict__ obs_out,
                                                            double nu) {
  extern __shared__ __attribute__((aligned(16))) double svgp_lds[];
  const int lda = mp + SVGP_LDS_PAD;
  double *a_s = svgp_lds, *w_s = a_s + SVGP_TILE * lda, *m_s = w_s + SVGP_TILE * lda;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t i0 = (int64_t)blockIdx.x * SVGP_TILE;
  const int np = (int)((tn - i0 < SVGP_TILE) ? (tn - i0) : SVGP_TILE);
  const double c = scalars[0];
  svgp_gather(At, ldat, nullptr, tn, i0, np, m, mp, lda, a_s);
  for (int k = t; k < mp; k += 256) m_s[k] = (k < m) ? mean[k] : 0.0;
  __syncthreads();
  svgp_tile_w(Ls, ldls, m, mp, lda, a_s, w_s);
  __syncthreads();
  for (int j = 0; j < SVGP_TILE / 4; ++j) {
    const int r = wave * (SVGP_TILE / 4) + j;
    const double mu = c + svgp_wave_dot(a_s + r * lda, m_s, mp);
    const double wn = svgp_wave_dot(w_s + r * lda, w_s + r * lda, mp);
    if (lane == 0 && r < np) {
      const double v = q[i0 + r] + wn;
      mean_out[i0 + r] = mu;
      var_out[i0 + r] = v;
      if (obs_out) {
        double obs;
        if (LIK == PLS_SVGP_BERNOULLI) {
          const double z = mu / sqrt(1.0 + v) * SVGP_INV_SQRT2;
          obs = (0.5 * erfc(-z)) * (0.5 * erfc(z));
        } else if (LIK == PLS_SVGP_STUDENT_T) {
          obs = v + svgp_noise<LIK>(scalars[1]) * (nu / (nu - 2.0));
        } else {
          obs = v + svgp_noise<LIK>(scalars[1]);
        }
        obs_out[i0 + r] = obs;
      }
    }
  }
}

// f(integral_constant<LIK>) for the likelihood of a validated descriptor: the one switch over the kernels' LIK parameter
template <class F>
static int for_likelihood(int likelihood, F &&f) {
  switch (likelihood) {
    case PLS_SVGP_BERNOULLI: return f(std::integral_constant<int, PLS_SVGP_BERNOULLI>{});
    case PLS_SVGP_STUDENT_T: return f(std::integral_constant<int, PLS_SVGP_STUDENT_T>{});
    default: return f(std::integral_constant<int, PLS_SVGP_GAUSSIAN>{});
  }
}

template <int LIK, bool GRAD>
static int svgp_launch_batch(const SvgpBatchArgs &ba, int64_t tiles, size_t lds, hipStream_t st) {
  if (int rc = ensure_lds<svgp_batch_kernel<LIK, GRAD>>(svgp_lds_bytes(SVGP_M_MAX))) return rc;
  hipLaunchKernelGGL((svgp_batch_kernel<LIK, GRAD>), dim3((unsigned)tiles), dim3(256), lds, st, ba);
  return PLS_OK;
}

// the likelihood of a validated descriptor as the kernels take it
static SvgpLikArgs svgp_lik_args(int likelihood, double deg_free) {
  SvgpLikArgs k{0.0, 0.0};
  if (likelihood == PLS_SVGP_STUDENT_T) {
    k.nu = deg_free;
    k.lgc = (std::lgamma(0.5 * (deg_free + 1.0)) - std::lgamma(0.5 * deg_free)) - 0.5 * std::log(deg_free * 3.14159265358979323846);
  }
  return k;
}

// the two launches of one evaluation over idx[0 .. b) (arguments already validated); ws laid out for THIS call's tiles
static int svgp_evaluate(const pls_svgp_desc *d, const SvgpLikArgs &lik, double *mean, double *Ls, int64_t ldls, double *scalars,
                         const int64_t *idx, int64_t b, bool grad, double *out, double *grad_m, double *grad_L, int64_t ldgl,
                         int update, int flags, double lr, double *loss_out, double *ws, hipStream_t st) {
  const int64_t mp = svgp_mp(d->m), tiles = svgp_tiles(b);
  SvgpBatchArgs ba{};
  ba.At = d->At, ba.ldat = d->ldat, ba.q = d->q, ba.y = d->y, ba.n = d->n, ba.m = (int)d->m, ba.mp = (int)mp;
  ba.mean = mean, ba.Ls = Ls, ba.ldls = ldls, ba.scalars = scalars, ba.idx = idx, ba.b = b;
  ba.kl = ws, ba.scal = ws + 4, ba.pm = ba.scal + 4 * tiles, ba.pG = ba.pm + tiles * mp;
  ba.lik = lik;
  const size_t lds = svgp_lds_bytes(mp);
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    const int rc = for_likelihood(d->likelihood, [&](auto tag) {
      constexpr int LIK = decltype(tag)::value;
      return grad ? svgp_launch_batch<LIK, true>(ba, tiles, lds, st) : svgp_launch_batch<LIK, false>(ba, tiles, lds, st);
    });
    if (rc) return rc;
  }
  if (int rc = check_launch("svgp_batch")) return rc;
  SvgpFinishArgs fa{};
  fa.m = (int)d->m, fa.mp = (int)mp, fa.rows = grad ? (int)d->m : 0, fa.n = d->n, fa.b = b, fa.tiles = tiles;
  fa.kl = ba.kl, fa.scal = ba.scal, fa.pm = ba.pm, fa.pG = ba.pG, fa.mean = mean, fa.Ls = Ls, fa.ldls = ldls;
  fa.scalars = scalars, fa.out = out, fa.grad_m = grad_m, fa.grad_L = grad_L, fa.ldgl = ldgl;
  fa.update = update, fa.flags = flags, fa.lik = d->likelihood, fa.lr = lr, fa.loss_out = loss_out;
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(svgp_finish_kernel, dim3((unsigned)(fa.rows + 1)), dim3(256), 0, st, fa);
  }
  return check_launch("svgp_finish");
}

// everything about a descriptor but its likelihood
static int svgp_check_sizes(const pls_svgp_desc *d, const char *who) {
  PLS_REQUIRE(d->n > 0 && d->m > 0, "%s: bad sizes n=%lld m=%lld", who, (long long)d->n, (long long)d->m);
  PLS_REQUIRE(d->m <= SVGP_M_MAX, "%s: %lld inducing points > %d are not supported", who, (long long)d->m, SVGP_M_MAX);
  PLS_REQUIRE(svgp_tiles(d->n) <= 2147483647, "%s: n=%lld too large", who, (long long)d->n);
  PLS_REQUIRE(d->At && d->q && d->y, "%s: NULL pointer in the descriptor", who);
  PLS_REQUIRE(d->ldat >= d->m, "%s: ldat < m", who);
  return PLS_OK;
}

static int svgp_check_desc(const pls_svgp_desc *d, const char *who) {
  PLS_REQUIRE(d, "%s: NULL descriptor", who);
  PLS_REQUIRE(d->likelihood == PLS_SVGP_GAUSSIAN, "%s: likelihood %d is not supported (PLS_SVGP_GAUSSIAN only)", who, d->likelihood);
  return svgp_check_sizes(d, who);
}

static int svgp_check_likelihood(int likelihood, double deg_free, const char *who) {
  PLS_REQUIRE(likelihood == PLS_SVGP_GAUSSIAN || likelihood == PLS_SVGP_BERNOULLI || likelihood == PLS_SVGP_STUDENT_T,
              "%s: unknown likelihood %d", who, likelihood);
  PLS_REQUIRE(likelihood != PLS_SVGP_STUDENT_T || (std::isfinite(deg_free) && deg_free > 2.0),
              "%s: the Student-t likelihood needs finite deg_free > 2, got %g", who, deg_free);
  return PLS_OK;
}

static int svgp_check_lik_desc(const pls_svgp_lik_desc *d, const char *who) {
  PLS_REQUIRE(d, "%s: NULL descriptor", who);
  if (int rc = svgp_check_likelihood(d->base.likelihood, d->deg_free, who)) return rc;
  return svgp_check_sizes(&d->base, who);
}

// the bodies of the entries, after the descriptor's own checks: `who` names the entry in the messages
static int svgp_elbo_grad(const pls_svgp_desc *desc, const SvgpLikArgs &lik, const char *who, const double *m, const double *L_s,
                          int64_t ldls, const double *scalars, const int64_t *idx, int64_t b, double *out, double *grad_m,
                          double *grad_L, int64_t ldgl, void *workspace, size_t workspace_bytes, void *stream) {
  PLS_REQUIRE(m && L_s && scalars && out, "%s: NULL pointer", who);
  PLS_REQUIRE(ldls >= desc->m, "%s: ldls < m", who);
  PLS_REQUIRE(b > 0 && svgp_tiles(b) <= 2147483647, "%s: bad batch length %lld", who, (long long)b);
  PLS_REQUIRE(idx || b <= desc->n, "%s: b=%lld > n=%lld without an index list", who, (long long)b, (long long)desc->n);
  PLS_REQUIRE(!grad_L || ldgl >= desc->m, "%s: ldgl < m", who);
  PLS_REQUIRE(workspace, "%s: NULL workspace", who);
  const bool grad = grad_m || grad_L;
  const size_t need = sizeof(double) * svgp_ws_doubles(svgp_tiles(b), svgp_mp(desc->m), grad);
  if (workspace_bytes < need)
    return fail(PLS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  PLS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  return svgp_evaluate(desc, lik, const_cast<double *>(m), const_cast<double *>(L_s), ldls, const_cast<double *>(scalars), idx, b,
                       grad, out, grad_m, grad_L, ldgl, 0, 0, 0.0, nullptr, static_cast<double *>(workspace), S(stream));
}

static int svgp_sgd_epoch(const pls_svgp_desc *desc, const SvgpLikArgs &lik, const char *who, double *m, double *L_s, int64_t ldls,
                          double *scalars, const int64_t *perm, int64_t batch_size, double lr, int32_t flags, double *loss_out,
                          void *workspace, size_t workspace_bytes, void *stream) {
  PLS_REQUIRE(m && L_s && scalars && perm && loss_out, "%s: NULL pointer", who);
  PLS_REQUIRE(ldls >= desc->m, "%s: ldls < m", who);
  PLS_REQUIRE(batch_size > 0, "%s: batch_size must be positive", who);
  PLS_REQUIRE((flags & ~(PLS_SVGP_TRAIN_MEAN | PLS_SVGP_TRAIN_NOISE)) == 0, "%s: unknown flag bits %d", who, flags);
  PLS_REQUIRE(workspace, "%s: NULL workspace", who);
  const int64_t bs = batch_size < desc->n ? batch_size : desc->n;
  const size_t need = pls_svgp_workspace_bytes(desc->n, desc->m, bs);
  if (workspace_bytes < need)
    return fail(PLS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  PLS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  double *ws = static_cast<double *>(workspace);
  for (int64_t first = 0; first < desc->n; first += bs) {
    const int64_t b = desc->n - first < bs ? desc->n - first : bs;
    if (int rc = svgp_evaluate(desc, lik, m, L_s, ldls, scalars, perm + first, b, true, nullptr, nullptr, nullptr, 0, 1, flags, lr,
                               nullptr, ws, S(stream)))
      return rc;
  }
  return svgp_evaluate(desc, lik, m, L_s, ldls, scalars, nullptr, desc->n, false, nullptr, nullptr, nullptr, 0, 0, 0, 0.0, loss_out,
                       ws, S(stream));
}

static int svgp_predict(int likelihood, double nu, const char *who, const double *m, const double *L_s, int64_t ldls,
                        const double *scalars, const double *At_test, int64_t ldat, const double *q_test, int64_t t, int64_t mdim,
                        double *mean_out, double *var_out, double *obs_out, void *stream) {
  PLS_REQUIRE(t > 0 && mdim > 0, "%s: bad sizes t=%lld m=%lld", who, (long long)t, (long long)mdim);
  PLS_REQUIRE(mdim <= SVGP_M_MAX, "%s: %lld inducing points > %d are not supported", who, (long long)mdim, SVGP_M_MAX);
  PLS_REQUIRE(svgp_tiles(t) <= 2147483647, "%s: t=%lld too large", who, (long long)t);
  PLS_REQUIRE(m && L_s && scalars && At_test && q_test && mean_out && var_out, "%s: NULL pointer", who);
  PLS_REQUIRE(ldls >= mdim && ldat >= mdim, "%s: ldls / ldat < m", who);
  hipStream_t st = S(stream);
  const int64_t mp = svgp_mp(mdim);
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    const int rc = for_likelihood(likelihood, [&](auto tag) -> int {
      constexpr int LIK = decltype(tag)::value;
      if (int rc = ensure_lds<svgp_predict_kernel<LIK>>(svgp_lds_bytes(SVGP_M_MAX))) return rc;
      hipLaunchKernelGGL((svgp_predict_kernel<LIK>), dim3((unsigned)svgp_tiles(t)), dim3(256), svgp_lds_bytes(mp), st, At_test, ldat,
                         q_test, t, (int)mdim, (int)mp, m, L_s, ldls, scalars, mean_out, var_out, obs_out, nu);
      return PLS_OK;
    });
    if (rc) return rc;
  }
  return check_launch("svgp_predict");
}

}  // namespace plship

using namespace plship;

extern "C" {

size_t pls_svgp_workspace_bytes(int64_t n, int64_t m, int64_t batch) {
  if (n <= 0 || m <= 0 || m > SVGP_M_MAX || batch <= 0) return 0;
  const int64_t mp = svgp_mp(m), tn = svgp_tiles(n), tb = svgp_tiles(batch);
  const size_t value = svgp_ws_doubles(tn > tb ? tn : tb, mp, false), grad = svgp_ws_doubles(tb, mp, true);
  return sizeof(double) * (value > grad ? value : grad);
}

// the Gaussian-only entries: the same bodies with the likelihood pinned
int pls_svgp_elbo_grad(const pls_svgp_desc *desc, const double *m, const double *L_s, int64_t ldls, const double *scalars,
                       const int64_t *idx, int64_t b, double *out, double *grad_m, double *grad_L, int64_t ldgl,
                       void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = svgp_check_desc(desc, "svgp_elbo_grad")) return rc;
  return svgp_elbo_grad(desc, SvgpLikArgs{0.0, 0.0}, "svgp_elbo_grad", m, L_s, ldls, scalars, idx, b, out, grad_m, grad_L, ldgl,
                        workspace, workspace_bytes, stream);
}

int pls_svgp_sgd_epoch(const pls_svgp_desc *desc, double *m, double *L_s, int64_t ldls, double *scalars, const int64_t *perm,
                       int64_t batch_size, double lr, int32_t flags, double *loss_out, void *workspace, size_t workspace_bytes,
                       void *stream) {
  if (int rc = svgp_check_desc(desc, "svgp_sgd_epoch")) return rc;
  return svgp_sgd_epoch(desc, SvgpLikArgs{0.0, 0.0}, "svgp_sgd_epoch", m, L_s, ldls, scalars, perm, batch_size, lr, flags, loss_out,
                        workspace, workspace_bytes, stream);
}

int pls_svgp_predict(const double *m, const double *L_s, int64_t ldls, const double *scalars, const double *At_test, int64_t ldat,
                     const double *q_test, int64_t t, int64_t mdim, double *mean_out, double *var_out, void *stream) {
  return svgp_predict(PLS_SVGP_GAUSSIAN, 0.0, "svgp_predict", m, L_s, ldls, scalars, At_test, ldat, q_test, t, mdim, mean_out,
                      var_out, nullptr, stream);
}

int pls_svgp_lik_elbo_grad(const pls_svgp_lik_desc *desc, const double *m, const double *L_s, int64_t ldls, const double *scalars,
                           const int64_t *idx, int64_t b, double *out, double *grad_m, double *grad_L, int64_t ldgl,
                           void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = svgp_check_lik_desc(desc, "svgp_lik_elbo_grad")) return rc;
  return svgp_elbo_grad(&desc->base, svgp_lik_args(desc->base.likelihood, desc->deg_free), "svgp_lik_elbo_grad", m, L_s, ldls,
                        scalars, idx, b, out, grad_m, grad_L, ldgl, workspace, workspace_bytes, stream);
}

int pls_svgp_lik_sgd_epoch(const pls_svgp_lik_desc *desc, double *m, double *L_s, int64_t ldls, double *scalars,
                           const int64_t *perm, int64_t batch_size, double lr, int32_t flags, double *loss_out, void *workspace,
                           size_t workspace_bytes, void *stream) {
  if (int rc = svgp_check_lik_desc(desc, "svgp_lik_sgd_epoch")) return rc;
  return svgp_sgd_epoch(&desc->base, svgp_lik_args(desc->base.likelihood, desc->deg_free), "svgp_lik_sgd_epoch", m, L_s, ldls,
                        scalars, perm, batch_size, lr, flags, loss_out, workspace, workspace_bytes, stream);
}

int pls_svgp_lik_predict(const pls_svgp_lik_desc *desc, const double *m, const double *L_s, int64_t ldls, const double *scalars,
                         const double *At_test, int64_t ldat, const double *q_test, int64_t t, int64_t mdim, double *mean_out,
                         double *var_out, double *obs_out, void *stream) {
  PLS_REQUIRE(desc, "svgp_lik_predict: NULL descriptor");
  if (int rc = svgp_check_likelihood(desc->base.likelihood, desc->deg_free, "svgp_lik_predict")) return rc;
  return svgp_predict(desc->base.likelihood, desc->deg_free, "svgp_lik_predict", m, L_s, ldls, scalars, At_test, ldat, q_test, t,
                      mdim, mean_out, var_out, obs_out, stream);
}

}  // extern "C"
