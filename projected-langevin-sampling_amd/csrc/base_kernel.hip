// The pairwise kernels of the base kernel (RBF-ARD, Matern 1/2, 3/2, 5/2, rational quadratic, periodic, locally periodic, trend
// plus seasonal; the Gram build also the linear kernel):
// pls_kernel_gram, pls_kernel_grad_sums, pls_kernel_mean.  The exact-GP path builds K with the first, differentiates with
// the second and predicts with the third, so the three evaluate a pair alike: the same pre-scaled points and distance
// sum (base_kernel.h), the same kappa (kernel_math.h).  The per-coordinate kinds (periodic, locally periodic, trend plus
// seasonal) have no single distance sum: unscaled points, one row of scales per parameter block in LDS, one sincospi per
// coordinate (base_kernel.h: pair_exponents, pair_factors_kept), and per term of the kind one exponential, one outputscale and
// one underflow decision.  Each kernel holds ONE branch for all of them, written over the kind's row of kind_facts.
#include <hip/hip_runtime.h>

#define PLS_SCALAR_POLY_CONSTANTS 1  // (fmath.h: the exp polynomial's constants as scalar operands)
#include "../../include/plship.h"
#include "base_kernel.h"

namespace plship {

typedef double double2m __attribute__((ext_vector_type(2)));

// k(x1, x2): a block covers PAIR_ROWS rows x PAIR_COLS columns; a thread owns one PAIR of columns (its two x2 points stay
// in registers, pre-scaled by 1/lengthscale) and walks down the rows, whose pre-scaled x1 points sit in LDS (broadcast
// reads).  Writes are 16 B per lane, 4 KiB contiguous per row and block: the kernel is bound by the 8*n1*n2 bytes it
// writes once the per-element work is ~35 fp64 instructions (D = 8).
template <int KIND, int D_MAX>
__global__ __launch_bounds__(256) void kernel_gram_kernel(const double *__restrict__ x1, int64_t n1,
                                                           const double *__restrict__ x2, int64_t n2, int d,
                                                           const double *__restrict__ lengthscale, double outputscale,
                                                           double *__restrict__ out, int64_t ldout) {
  __shared__ double scales[scale_rows(KIND)][D_MAX];                    // (base_kernel.h: stage_scales)
  __shared__ __attribute__((aligned(16))) double a_s[PAIR_ROWS][D_MAX];  // rows of x1 (pre-scaled, zero-padded)
  const double(&inv_ls)[D_MAX] = scales[0];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * PAIR_ROWS;
  const int nrows = (int)((n1 - row0 < PAIR_ROWS) ? (n1 - row0) : PAIR_ROWS);
  stage_scales<KIND>(scales, lengthscale, d);
  const PairShape sh = load_pair_shape<KIND>(lengthscale, d);
  __syncthreads();
  stage_rows<KIND>(a_s, x1, row0, nrows, d, inv_ls);
  __syncthreads();
  const int64_t col = ((int64_t)blockIdx.x * 256 + t) * 2;
  if (col >= n2) return;
  const bool two = col + 1 < n2;
  double b0[D_MAX], b1[D_MAX];
#pragma unroll
  for (int k = 0; k < D_MAX; ++k) {
    b0[k] = (k < d) ? pair_scaled<KIND>(x2[col * d + k], inv_ls[k]) : 0.0;
    b1[k] = (k < d && two) ? pair_scaled<KIND>(x2[(col + 1) * d + k], inv_ls[k]) : 0.0;
  }
  const bool vec = two && ((ldout & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  double *dst = out + row0 * ldout + col;
#pragma unroll 2
  for (int r = 0; r < nrows; ++r, dst += ldout) {
    double s0 = 0.0, s1 = 0.0;
    if constexpr (periodic_like(KIND)) {
      double q0, q1;
      pair_exponents<KIND>(a_s[r], b0, b1, scales, s0, q0, s1, q1);
      s0 = coord_entry<KIND>(s0, q0, outputscale, sh);
      s1 = coord_entry<KIND>(s1, q1, outputscale, sh);
    } else if (KIND != PLS_KERNEL_LINEAR) {
      pair_dist2(a_s[r], b0, b1, s0, s1);
      s0 = gram_entry<KIND>(s0, sh, outputscale);
      s1 = gram_entry<KIND>(s1, sh, outputscale);
    } else {
#pragma unroll
      for (int k = 0; k < D_MAX; ++k) {
        const double a = a_s[r][k];
        s0 = fma(a, b0[k], s0);
        s1 = fma(a, b1[k], s1);
      }
    }
    if (vec) {
      *reinterpret_cast<double2m *>(dst) = double2m{s0, s1};
    } else {
      dst[0] = s0;
      if (two) dst[1] = s1;
    }
  }
}

// The reduction over the n x n pair matrix, laid out as kernel_gram_kernel (a thread owns a PAIR of columns and walks down
// the rows in LDS).  P is read once, 16 B per lane where ldp is even and P is 16-byte aligned.  With B = 1 + the kind's
// per-dimension blocks a thread carries 1 + B D_MAX + scalars accumulators: the kappa sum, B blocks of D_MAX, the scalars.
//   out[0]     = sum_ij W_ij kappa_ij                  (kappa: the kernel without its outputscale)
//   out[1 + k] = sum_ij W_ij dK_ij / d log l_k         (RBF: s exp(-r^2/2) e_k^2;  Matern: s q(t) exp(-t) 2 nu e_k^2 with
//                                                       q = 1/t, 1, (1 + t)/3 for nu = 1/2, 3/2, 5/2;  RQ: s kappa / (1 + u) e_k^2;
//                                                       e_k = (x_ik - x_jk)/l_k)
//   out[1 + d] = sum_ij W_ij dK_ij / d log alpha       (RQ only: s alpha kappa (u / (1 + u) - log1p(u)), u = r^2 / (2 alpha))
//   per-coordinate kinds: out[1 + j d + k] = sum_ij W_ij s kappa f_jk, f_jk coordinate k's factor of block j's parameter
//   (kernel_math.h: pair_coord), s kappa the term's that the block belongs to.  Trend plus seasonal: block 0 (l) with s_t kappa_t,
//   which is also out[0]'s kappa; blocks 1 to 3 (m, lambda, p) with s_s kappa_s, and out[1 + 4 d] = sum_ij W_ij s_s kappa_s
// with W = alpha alpha^T - P; no atomics: per thread down its rows, then the workgroup sum below, then the workgroups'
// partial rows in ascending order (a second one-workgroup launch).
template <int KIND, int D_MAX>
__global__ __launch_bounds__(256) void kernel_grad_sums_kernel(const double *__restrict__ x, int64_t n, int d,
                                                                const double *__restrict__ lengthscale, double outputscale,
                                                                const double *__restrict__ alpha, const double *__restrict__ P,
                                                                int64_t ldp, double *__restrict__ partials) {
  constexpr KindFacts FACTS = kind_facts(KIND);
  __shared__ double scales[scale_rows(KIND)][D_MAX];  // (base_kernel.h: stage_scales)
  __shared__ __attribute__((aligned(16))) double a_s[PAIR_ROWS][D_MAX];
  __shared__ double al_s[PAIR_ROWS];
  const double(&inv_ls)[D_MAX] = scales[0];
  constexpr bool SHAPE = KIND == PLS_KERNEL_RQ;
  // the sums of the B per-dimension blocks, D_MAX apart, then the scalars': acc[1 + B D_MAX + j], written to slot 1 + B d + j
  constexpr int B = 1 + FACTS.blocks, NACC = 1 + B * D_MAX + FACTS.scalars;
  __shared__ double red[4][NACC];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * PAIR_ROWS;
  const int nrows = (int)((n - row0 < PAIR_ROWS) ? (n - row0) : PAIR_ROWS);
  stage_scales<KIND>(scales, lengthscale, d);
  const PairShape sh = load_pair_shape<KIND>(lengthscale, d);
  if (t < PAIR_ROWS) al_s[t] = (t < nrows) ? alpha[row0 + t] : 0.0;
  __syncthreads();
  stage_rows<KIND>(a_s, x, row0, nrows, d, inv_ls);
  __syncthreads();
  const int64_t col = ((int64_t)blockIdx.x * 256 + t) * 2;
  const bool one = col < n, two = col + 1 < n;
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  if (one) {
    double b0[D_MAX], b1[D_MAX];
#pragma unroll
    for (int k = 0; k < D_MAX; ++k) {
      b0[k] = (k < d) ? pair_scaled<KIND>(x[col * d + k], inv_ls[k]) : 0.0;
      b1[k] = (k < d && two) ? pair_scaled<KIND>(x[(col + 1) * d + k], inv_ls[k]) : 0.0;
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
      if constexpr (FACTS.per_coord) {
        // One column at a time: the factors of its first KEEP coordinates live in registers between the sums and the
        // accumulation, the others are evaluated again afterwards (base_kernel.h: factors_kept).  The kind's last term is
        // the periodic one, over the blocks from FIRST on; the term in front of it, if any, is the trend's, over block 0.
        // Each term takes its own underflow decision, and a dead one adds nothing to its sums.
        constexpr int KEEP = factors_kept(KIND, D_MAX), FIRST = FACTS.terms - 1;
        auto column = [&](const double (&b)[D_MAX], double w, bool have) {
          double f[B][KEEP], s2, q, kt, ks;
          pair_factors_kept<KIND, KEEP>(a_s[r], b, scales, s2, q, f);
          const bool live_t = FIRST > 0 && trend_kappa(s2, kt) && have, live_s = periodic_kappa(q, ks) && have;
          if constexpr (FIRST > 0) {
            static_assert(KEEP == D_MAX && FACTS.scalars == 1, "every factor of the trend's is kept; the last term's outputscale");
            if (live_t) {
              const double gw = w * (outputscale * kt);
              acc[0] = fma(w, kt, acc[0]);
#pragma unroll
              for (int k = 0; k < D_MAX; ++k) acc[1 + k] = fma(gw, f[0][k], acc[1 + k]);
            }
          }
          if (live_s) {
            // s kappa of the term: under the kind's outputscale, or under its own, which has its kappa sum behind the blocks
            const double sk = (FIRST > 0 ? sh.alpha : outputscale) * ks;
            const double gw = w * sk;
            if constexpr (FIRST > 0) acc[1 + B * D_MAX] = fma(w, sk, acc[1 + B * D_MAX]);
            else acc[0] = fma(w, ks, acc[0]);
#pragma unroll
            for (int k = 0; k < KEEP; ++k)
#pragma unroll
              for (int j = FIRST; j < B; ++j) acc[1 + j * D_MAX + k] = fma(gw, f[j][k], acc[1 + j * D_MAX + k]);
#pragma unroll
            for (int k = KEEP; k < D_MAX; ++k) {
              double sc[B], fk[B], unused = 0.0, delta = a_s[r][k] - b[k];
              // (opaque to the optimiser: merged with the first evaluation, its values would stay live after all)
              asm volatile("" : "+v"(delta));
              scale_column(scales, k, sc);
              pair_coord<KIND, true>(delta, sc, unused, fk);
#pragma unroll
              for (int j = FIRST; j < B; ++j) acc[1 + j * D_MAX + k] = fma(gw, fk[j], acc[1 + j * D_MAX + k]);
            }
          }
        };
        column(b0, w0, true);
        column(b1, w1, two);
      } else {
        double s0, s1;
        pair_dist2(a_s[r], b0, b1, s0, s1);
        double kap0, g0, ga0, kap1, g1, ga1;
        const bool live0 = pair_factors<KIND>(s0, sh, kap0, g0, ga0);
        const bool live1 = pair_factors<KIND>(s1, sh, kap1, g1, ga1) && two;
        if (live0) {
          const double gw = w0 * (outputscale * g0);
          acc[0] = fma(w0, kap0, acc[0]);
          if constexpr (SHAPE) acc[D_MAX + 1] = fma(w0, outputscale * ga0, acc[D_MAX + 1]);
#pragma unroll
          for (int k = 0; k < D_MAX; ++k) {
            const double e = a_s[r][k] - b0[k];
            acc[1 + k] = fma(gw, e * e, acc[1 + k]);
          }
        }
        if (live1) {
          const double gw = w1 * (outputscale * g1);
          acc[0] = fma(w1, kap1, acc[0]);
          if constexpr (SHAPE) acc[D_MAX + 1] = fma(w1, outputscale * ga1, acc[D_MAX + 1]);
#pragma unroll
          for (int k = 0; k < D_MAX; ++k) {
            const double e = a_s[r][k] - b1[k];
            acc[1 + k] = fma(gw, e * e, acc[1 + k]);
          }
        }
      }
    }
  }
  // workgroup sum in a fixed order: xor butterfly inside each wave, then (w0 + w1) + (w2 + w3)
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((t & 63) == 0) red[t >> 6][k] = v;
  }
  __syncthreads();
  const int nsums = 1 + B * d + FACTS.scalars;
  if (t < nsums) {
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    // slot t of the partial row: the kappa sum, the blocks d apart (D_MAX apart in acc), the scalars.  The distance-sum kinds
    // (B = 1) keep that formula's values in the form their machine code was built from.
    const int k = !FACTS.per_coord ? ((SHAPE && t == d + 1) ? D_MAX + 1 : t)
                  : (t > B * d)    ? 1 + B * D_MAX + (t - 1 - B * d)
                  : (t > 0)        ? 1 + ((t - 1) / d) * D_MAX + (t - 1) % d
                                   : 0;
    partials[blk * nsums + t] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// out[k] = the partial rows of the workgroups added in ascending order
__global__ __launch_bounds__(128) void grad_sums_finish_kernel(const double *__restrict__ partials, int64_t nblocks, int nsums,
                                                                double *__restrict__ out) {
  const int k = threadIdx.x;
  if (k >= nsums) return;
  double s = 0.0;
  for (int64_t b = 0; b < nblocks; ++b) s += partials[b * nsums + k];
  out[k] = s;
}

int grad_sums_launch(int kind, const double *x, int64_t n, int d, const double *lengthscale, double outputscale,
                     const double *alpha, const double *P, int64_t ldp, double *out, double *partials, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(n, PAIR_COLS), (unsigned)cdiv(n, PAIR_ROWS));
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    for_kind_dmax<false>(kind, d, [&](auto k, auto dm) {
      hipLaunchKernelGGL((kernel_grad_sums_kernel<decltype(k)::value, decltype(dm)::value>), grid, dim3(256), 0, st, x, n, d,
                         lengthscale, outputscale, alpha, P, ldp, partials);
      return 0;
    });
  }
  if (int rc = check_launch("kernel_grad_sums")) return rc;
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    hipLaunchKernelGGL(grad_sums_finish_kernel, dim3(1), dim3(128), 0, st, partials, grad_sums_blocks(n),
                       (int)grad_sums_count(kind, d), out);
  }
  return check_launch("grad_sums_finish");
}

// ---- the predictive mean without the cross-Gram matrix -------------------------------------------------------------
// out[i] = mean + outputscale * sum_j kappa(xt_i, x_j) alpha_j.  A workgroup owns MEAN_POINTS = 64 test points: lane l of
// EVERY wave holds test point 64 b + l in registers (pre-scaled by 1/lengthscale, zero-padded to D_MAX); the training
// points pass through LDS in chunks of mean_chunk(D_MAX) (pre-scaled, broadcast reads) and wave w takes the points
// j = w, w + 4, w + 8, ... (the chunk length is a multiple of 4, so the split is j mod 4 whatever the chunk).  Each thread
// adds its terms in ascending j into one accumulator (trend plus seasonal: one per term, out[i] = fma(s_t, A_t, fma(s_s, A_s,
// mean))); the four waves' sums meet in LDS as (w0 + w1) + (w2 + w3).  A lane
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
  constexpr bool TWO_TERMS = kind_facts(KIND).terms == 2;
  __shared__ double scales[scale_rows(KIND)][D_MAX];  // (base_kernel.h: stage_scales)
  __shared__ __attribute__((aligned(16))) double a_s[CHUNK][D_MAX];
  __shared__ double al_s[CHUNK];
  __shared__ double red[4][MEAN_POINTS];
  __shared__ double red_s[TWO_TERMS ? 4 : 1][MEAN_POINTS];  // (trend plus seasonal: the seasonal term's sums)
  const double(&inv_ls)[D_MAX] = scales[0];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  stage_scales<KIND>(scales, lengthscale, d);
  const PairShape sh = load_pair_shape<KIND>(lengthscale, d);
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
        b[k] = pair_scaled<KIND>(v.x, inv_ls[k]);
        if (k + 1 < D_MAX) b[k + 1] = pair_scaled<KIND>(v.y, inv_ls[(k + 1) % D_MAX]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < D_MAX; ++k) b[k] = (k < d) ? pair_scaled<KIND>(row[k], inv_ls[k]) : 0.0;
    }
  }
  const bool xvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  double acc = 0.0;
  [[maybe_unused]] double acc_s = 0.0;  // (trend plus seasonal: acc holds the trend's sum A_t, acc_s the seasonal A_s)
  for (int64_t j0 = 0; j0 < n; j0 += CHUNK) {
    const int nrows = (int)((n - j0 < CHUNK) ? (n - j0) : CHUNK);
    const int len = nrows * d;  // <= 512 * 64
    const double *src = x + j0 * d;
    if (xvec) {
      for (int p = tid; 2 * p < len; p += 256) {
        const int e = 2 * p;
        if (e + 1 < len) {
          const double2m v = *reinterpret_cast<const double2m *>(src + e);
          a_s[e / d][e % d] = pair_scaled<KIND>(v.x, inv_ls[e % d]);
          a_s[(e + 1) / d][(e + 1) % d] = pair_scaled<KIND>(v.y, inv_ls[(e + 1) % d]);
        } else {
          a_s[e / d][e % d] = pair_scaled<KIND>(src[e], inv_ls[e % d]);
        }
      }
    } else {
      for (int e = tid; e < len; e += 256) a_s[e / d][e % d] = pair_scaled<KIND>(src[e], inv_ls[e % d]);
    }
    for (int r = tid; r < nrows; r += 256) al_s[r] = alpha[j0 + r];
    __syncthreads();
#pragma unroll 2
    for (int r = w; r < nrows; r += 4) {
      double kap;
      bool alive;
      if constexpr (periodic_like(KIND)) {
        double s2, q;
        pair_exponents<KIND>(a_s[r], b, scales, s2, q);
        if constexpr (TWO_TERMS) {
          double ks;
          alive = trend_kappa(s2, kap);
          if (periodic_kappa(q, ks)) acc_s = fma(ks, al_s[r], acc_s);
        } else alive = periodic_kappa(q, kap);
      } else alive = pair_kappa<KIND>(pair_dist2(a_s[r], b), sh, kap);
      if (alive) acc = fma(kap, al_s[r], acc);
    }
    __syncthreads();
  }
  red[w][lane] = acc;
  if constexpr (TWO_TERMS) red_s[w][lane] = acc_s;
  __syncthreads();
  if constexpr (TWO_TERMS) {
    if (w == 0 && live)
      out[i] = fma(outputscale, (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]),
                   fma(sh.alpha, (red_s[0][lane] + red_s[1][lane]) + (red_s[2][lane] + red_s[3][lane]), mean));
  } else if (w == 0 && live) out[i] = fma(outputscale, (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]), mean);
}

// the one launch of pls_kernel_mean (arguments already validated, t > 0)
static int kernel_mean_launch(int kind, const double *x, int64_t n, int d, const double *lengthscale, double outputscale,
                              double mean, const double *alpha, const double *xt, int64_t t, double *out, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(t, (int64_t)MEAN_POINTS));
  {
    LaunchScope scope(PLS_TAG_OTHER, st);
    for_kind_dmax<false>(kind, d, [&](auto k, auto dm) {
      hipLaunchKernelGGL((kernel_mean_kernel<decltype(k)::value, decltype(dm)::value>), grid, dim3(256), 0, st, x, n, d,
                         lengthscale, outputscale, mean, alpha, xt, t, out);
      return 0;
    });
  }
  return check_launch("kernel_mean");
}

int gp_check_shared(const char *who, int32_t kernel_kind, int64_t n, int64_t d, const int64_t *classes, const void *workspace,
                    size_t workspace_bytes, size_t need, int align) {
  PLS_REQUIRE(kernel_kind != PLS_KERNEL_LINEAR, "%s: the linear kernel has no lengthscale or outputscale to learn", who);
  PLS_REQUIRE(stationary_kind(kernel_kind), "%s: unknown kernel kind %d", who, kernel_kind);
  if (classes)
    PLS_REQUIRE(n > 0 && d > 0 && *classes > 0, "%s: bad sizes n=%lld d=%lld classes=%lld", who, (long long)n, (long long)d,
                (long long)*classes);
  PLS_REQUIRE(n > 0 && d > 0, "%s: bad sizes n=%lld d=%lld", who, (long long)n, (long long)d);
  if (int rc = check_kind_dim(who, kernel_kind, d)) return rc;
  PLS_REQUIRE(cdiv(n, PAIR_ROWS) <= 65535, "%s: n=%lld too large", who, (long long)n);
  PLS_REQUIRE(workspace, "%s: NULL workspace", who);
  if (workspace_bytes < need)
    return fail(PLS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  PLS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & (uintptr_t)(align - 1)) == 0, "%s: workspace must be %d-byte aligned", who,
              align);
  return PLS_OK;
}

}  // namespace plship

using namespace plship;

extern "C" {

int pls_kernel_gram(int32_t kernel_kind, const double *x1, int64_t n1, const double *x2, int64_t n2, int64_t d,
                    const double *lengthscale, double outputscale, double *out, int64_t ldout, void *stream) {
  PLS_REQUIRE(kernel_kind == PLS_KERNEL_LINEAR || stationary_kind(kernel_kind), "unknown kernel kind %d", kernel_kind);
  PLS_REQUIRE(x1 && x2 && out, "kernel_gram: NULL pointer");
  PLS_REQUIRE(n1 >= 0 && n2 >= 0 && d >= 1, "kernel_gram: bad sizes n1=%lld n2=%lld d=%lld", (long long)n1, (long long)n2, (long long)d);
  if (int rc = check_kind_dim("kernel_gram", kernel_kind, d)) return rc;
  PLS_REQUIRE(ldout >= n2, "kernel_gram: ldout < n2");
  PLS_REQUIRE(kernel_kind == PLS_KERNEL_LINEAR || lengthscale, "kernel_gram: kernel kind %d needs lengthscale", kernel_kind);
  if (n1 == 0 || n2 == 0) return PLS_OK;
  PLS_REQUIRE(cdiv(n2, PAIR_COLS) <= 0x7fffffff, "kernel_gram: n2 too large");
  const int64_t max_rows = 65535LL * PAIR_ROWS;  // gridDim.y <= 65535: taller Gram matrices go in row slabs
  for (int64_t r0 = 0; r0 < n1; r0 += max_rows) {
    const int64_t rows = (n1 - r0 < max_rows) ? n1 - r0 : max_rows;
    const dim3 grid((unsigned)cdiv(n2, PAIR_COLS), (unsigned)cdiv(rows, PAIR_ROWS));
    LaunchScope scope(PLS_TAG_KERNEL_GRAM, S(stream));
    for_kind_dmax<true>(kernel_kind, (int)d, [&](auto k, auto dm) {
      hipLaunchKernelGGL((kernel_gram_kernel<decltype(k)::value, decltype(dm)::value>), grid, dim3(256), 0, S(stream),
                         x1 + r0 * d, rows, x2, n2, (int)d, lengthscale, outputscale, out + r0 * ldout, ldout);
      return 0;
    });
    int rc = check_launch("kernel_gram");
    if (rc) return rc;
  }
  return PLS_OK;
}

size_t pls_kernel_grad_sums_workspace_bytes_kind(int32_t kernel_kind, int64_t n, int64_t d) {
  return (stationary_kind(kernel_kind) && n > 0 && d > 0 && d <= kind_d_max(kernel_kind)) ? grad_sums_workspace_bytes(kernel_kind, n, d) : 0;
}
size_t pls_kernel_grad_sums_workspace_bytes(int64_t n, int64_t d) {
  return pls_kernel_grad_sums_workspace_bytes_kind(PLS_KERNEL_RBF_ARD, n, d);
}

int pls_kernel_grad_sums(int32_t kernel_kind, const double *x, int64_t n, int64_t d, const double *lengthscale,
                         double outputscale, const double *alpha, const double *P, int64_t ldp, double *out, void *workspace,
                         size_t workspace_bytes, void *stream) {
  if (int rc = gp_check_shared("kernel_grad_sums", kernel_kind, n, d, nullptr, workspace, workspace_bytes,
                               pls_kernel_grad_sums_workspace_bytes_kind(kernel_kind, n, d), 8))
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
  if (int rc = check_kind_dim("kernel_mean", kernel_kind, d)) return rc;
  PLS_REQUIRE(cdiv(t, (int64_t)MEAN_POINTS) <= 2147483647, "kernel_mean: t=%lld too large", (long long)t);
  if (t == 0) return PLS_OK;
  PLS_REQUIRE(x && lengthscale && alpha && xt && out, "kernel_mean: NULL pointer");
  return kernel_mean_launch(kernel_kind, x, n, (int)d, lengthscale, outputscale, mean, alpha, xt, t, out, S(stream));
}

}  // extern "C"
