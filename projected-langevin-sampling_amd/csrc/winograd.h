// One level of Strassen-Winograd for the back-projection D = A G of the general step: the forward GEMM
// on paired tiles with epilogues that leave G as the seven right-hand operand planes, and its launcher.  The products, the
// left-hand planes and the update that combines the products live in plship.hip.
//
// With A = At^T (M_k x N) and G (N x J) cut in halves -- A_ab: half a of M_k, half b of N; G_bc: half b of N, half c of J:
//   S1 = A21 + A22   S2 = S1 - A11   S3 = A11 - A21   S4 = A12 - S2        (constant: built from At)
//   T1 = G12 - G11   T2 = G22 - T1   T3 = G22 - G12   T4 = T2 - G21        (per step: the forward epilogue)
//   P1 = A11 G11  P2 = A12 G21  P3 = S4 G22  P4 = A22 T4  P5 = S1 T1  P6 = S2 T2  P7 = S3 T3
//   D11 = P1 + P2   W = P1 + P6   D21 = (W + P7) - P4   D22 = (W + P7) + P5   D12 = (W + P5) + P3
// Seven products of half size instead of the eight a blocked product takes: 7/8 of the matrix-pipe work.
#pragma once
#include "cost_device.h"
#include "gemm_tn_f64.h"

namespace plship {

// The right-hand planes of one chunk: kWinoPlanes planes of (paired rows x J/2), `plane` doubles apart, leading dimension ldq.
enum WinoPlane { WQ_G11 = 0, WQ_G21 = 1, WQ_G22 = 2, WQ_T1 = 3, WQ_T2 = 4, WQ_T3 = 5, WQ_T4 = 6, kWinoPlanes = 7 };

// acc holds G of a wave's paired block (rows prow0 + 16 (ta & 1) + 4 r + (lane >> 4) of half ta >> 1, columns
// pcol0 + 16 (tb & 1) + (lane & 15) of half tb >> 1): every lane owns the four quadrant partners of its elements.
template <int TI, int TJ>
__device__ __forceinline__ void winograd_store(const AccFrag<TI, TJ> &acc, double *Q, int64_t ldq, int64_t plane, int64_t prow0,
                                               int64_t pcol0, int lane, int64_t I, int64_t J) {
  static_assert(TI == 4 && TJ == 4, "paired 64 x 64 wave blocks");
  const int q = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t prow = prow0 + 16 * ta + 4 * r + q;
#pragma unroll
      for (int tb = 0; tb < 2; ++tb) {
        const int64_t pcol = pcol0 + 16 * tb + c16;
        const double g11 = acc.v[ta][tb][r], g12 = acc.v[ta][tb + 2][r];
        const double g21 = acc.v[ta + 2][tb][r], g22 = acc.v[ta + 2][tb + 2][r];
        const double t1 = g12 - g11, t2 = g22 - t1, t3 = g22 - g12, t4 = t2 - g21;
        if (prow < I && pcol < J) {
          double *o = Q + prow * ldq + pcol;
          o[WQ_G11 * plane] = g11;
          o[WQ_G21 * plane] = g21;
          o[WQ_G22 * plane] = g22;
          o[WQ_T1 * plane] = t1;
          o[WQ_T2 * plane] = t2;
          o[WQ_T3 * plane] = t3;
          o[WQ_T4 * plane] = t4;
        }
      }
    }
}

// Gaussian cost, identity link: G = fma(F, 1/sigma2, -y/sigma2) (the formula of EpiGaussDeriv) in the MFMA registers.
// vpart (optional): per wave row (32 paired rows = 64 data rows) and data column, sum of cost = G^2 sigma2 / 2 over its rows.
struct EpiWinoGauss {
  static constexpr int kTag = PLS_TAG_GEMM_COST_DERIV;
  double *Q;
  int64_t ldq, plane;
  const double *y;  // data rows of the chunk: paired row p is data row p (first half) and p + pair_i (second half)
  int64_t pair_i, pair_j;
  double inv_noise;
  double *vpart;
  int64_t ldp;
  __device__ void apply(AccFrag<4, 4> &acc, int64_t prow0, int64_t pcol0, int lane, int, int64_t I, int64_t J, double *) const {
    const int q = lane >> 4, c16 = lane & 15;
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t prow = prow0 + 16 * (ta & 1) + 4 * r + q;
        const bool ok = prow < I;
        const double yv = ok ? -inv_noise * y[prow + (ta >> 1) * pair_i] : 0.0;
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
          const double g = fma(acc.v[ta][tb][r], inv_noise, yv);
          acc.v[ta][tb][r] = g;
          if (vpart && ok) sq[tb] = fma(g, g, sq[tb]);
        }
      }
    if (vpart) {
      const double half_s2 = 0.5 / inv_noise;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) {
        double t = sq[tb];
        t += __shfl_xor(t, 16);
        t += __shfl_xor(t, 32);  // the four lane groups hold rows (lane >> 4) + 4 r of the same column
        const int64_t pcol = pcol0 + 16 * (tb & 1) + c16;
        if (lane < 16 && prow0 < I && pcol < J) vpart[(prow0 / 32) * ldp + (tb >> 1) * pair_j + pcol] = t * half_s2;
      }
    }
    winograd_store<4, 4>(acc, Q, ldq, plane, prow0, pcol0, lane, I, J);
  }
};

// Any other cost: G = cost'(y, F) through the wave's LDS slab, 16 rows at a time, so that the per-element code exists once
// (see epilogue_row_pairs): the slab is written in the MFMA layout, each lane walks one column down its 16 rows and writes G
// back in place, and the slab returns to the registers for the combination.  vpart as in EpiWinoGauss (cost values).
template <int COST, int LINK>
struct EpiWinoCost {
  static constexpr int kTag = PLS_TAG_GEMM_COST_DERIV;
  double *Q;
  int64_t ldq, plane;
  const double *y;
  int64_t pair_i, pair_j;
  CostP cp;
  double *vpart;
  int64_t ldp;
  __device__ void apply(AccFrag<4, 4> &acc, int64_t prow0, int64_t pcol0, int lane, int wave, int64_t I, int64_t J,
                        double *lds) const {
    constexpr int STRIDE = 64 + EPI_PAD;
    CostP cp = this->cp;
    if constexpr (COST >= 0) {
      cp.cost = COST;
      if constexpr (LINK >= 0) cp.link = LINK;
    }
    const int q = lane >> 4, c16 = lane & 15;
    double *w = lds + wave * 16 * STRIDE;
    // lane l holds y of the wave's row slot l: block l >> 4 (half (l >> 5)), row l & 15 of it
    const int64_t lrow = prow0 + 16 * ((lane >> 4) & 1) + (lane & 15);
    const double yl = lrow < I ? y[lrow + (lane >> 5) * pair_i] : 0.0;
    double s = 0.0;
    auto slab = [&](auto ta_tag, bool to_lds) {
      constexpr int ta = decltype(ta_tag)::value;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double &x = w[(4 * r + q) * STRIDE + tb * 16 + c16];
          if (to_lds)
            x = acc.v[ta][tb][r];
          else
            acc.v[ta][tb][r] = x;
        }
    };
    auto pass = [&](int ta, bool to_lds) {
      switch (ta) {
        case 0: slab(std::integral_constant<int, 0>{}, to_lds); break;
        case 1: slab(std::integral_constant<int, 1>{}, to_lds); break;
        case 2: slab(std::integral_constant<int, 2>{}, to_lds); break;
        default: slab(std::integral_constant<int, 3>{}, to_lds); break;
      }
    };
#pragma unroll 1
    for (int ta = 0; ta < 4; ++ta) {
      pass(ta, true);
      __builtin_amdgcn_wave_barrier();  // (the slab is private to the wave; its LDS operations run in issue order)
#pragma unroll 1
      for (int rr = 0; rr < 16; ++rr) {
        const double yv = __shfl(yl, ta * 16 + rr);
        double &x = w[rr * STRIDE + lane];
        const double f = x;
        x = cost_deriv_of<COST>(cp, yv, f);
        if (vpart && prow0 + 16 * (ta & 1) + rr < I) s += cost_value_of<COST>(cp, yv, f);
      }
      __builtin_amdgcn_wave_barrier();
      pass(ta, false);
    }
    if (vpart) {
      const int64_t pcol = pcol0 + 16 * ((lane >> 4) & 1) + c16;
      if (prow0 < I && pcol < J) vpart[(prow0 / 32) * ldp + (lane >> 5) * pair_j + pcol] = s;
    }
    winograd_store<4, 4>(acc, Q, ldq, plane, prow0, pcol0, lane, I, J);
  }
};

// The forward GEMM on paired tiles: F = Lf^T V over paired rows [0, I) (data rows p and p + pair_i of Lf) and paired columns
// [0, J) (particle columns c and c + pair_j), its epilogue leaving the seven planes.  The k-loop, its LDS layout and its DMA
// are gemm_tn_mainloop's; needs 16-byte aligned operands, even leading dimensions and an even pair_i / pair_j.
template <class Epi>
__global__ __launch_bounds__(256, 2) void gemm_paired_kernel(GemmShape g, Epi epi) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int tile_i, tile_j;
  gemm_tile_coords(blockIdx.x, g.nti, g.ntj, tile_i, tile_j);
  const int64_t i0 = (int64_t)tile_i * 64, j0 = (int64_t)tile_j * 64;
  AccFrag<4, 4> acc;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc.v[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wr = wave >> 1, wc = wave & 1;
  if (i0 + 64 > g.I || j0 + 64 > g.J)
    gemm_tn_mainloop<128, 128, 64, 64, 16, true, true, true, 4, 16, 4, 4, true>(g, i0, j0, lds, acc, wr * 64);
  else
    gemm_tn_mainloop<128, 128, 64, 64, 16, true, false, true, 4, 16, 4, 4, true>(g, i0, j0, lds, acc, wr * 64);
  epi.apply(acc, i0 + 32 * wr, j0 + 32 * wc, lane, wave, g.I, g.J, lds);
}

// paired forward of one chunk: Lf (K x 2 pair_i, data rows of the chunk at Lf and Lf + pair_i), V (K x 2 pair_j)
template <class Epi>
static int launch_gemm_paired(const double *Lf, int64_t ldlf, int64_t pair_i, const double *V, int64_t ldv, int64_t pair_j,
                              int64_t rows, int64_t K, const Epi &epi, hipStream_t st) {
  constexpr size_t lds_bytes = gemm_tile_lds_bytes(128, 128, 16);
  constexpr auto kern = gemm_paired_kernel<Epi>;
  // (the second halves sit pair_i / pair_j columns into the rows: the DMA's lane offsets carry them)
  if (int rc = gemm_dma_check(Lf, ldlf, pair_i + rows, V, ldv, 2 * pair_j)) return rc;
  if (int rc = ensure_lds<kern>(lds_bytes)) return rc;
  GemmShape g{Lf, ldlf, V, ldv, rows, pair_j, K, 0, 0, 0, 0};
  g.pair_i = pair_i;
  g.pair_j = pair_j;
  g.nti = (int)cdiv(rows, 64);
  g.ntj = (int)cdiv(pair_j, 64);
  const int64_t nwg = (int64_t)g.nti * g.ntj;
  if (nwg <= 0) return PLS_OK;
  if (nwg > 0x7fffffff) return fail(PLS_ERR_INVALID_ARGUMENT, "gemm_paired: too many tiles");
  {
    LaunchScope scope(Epi::kTag, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), lds_bytes, st, g, epi);
  }
  return check_launch("gemm_paired");
}

// Forward GEMM of one chunk of paired rows + cost derivative, leaving the seven planes Q (ldq = pair_j, `plane` doubles apart)
// and, with vpart, cdiv(rows, 32) partial rows of the cost value.  Dispatches on (cost, link); defined in gemm_cost.hip.
int launch_cost_deriv_paired(const double *Lf, int64_t ldlf, int64_t pair_i, const double *V, int64_t ldv, int64_t pair_j,
                             int64_t rows, int64_t kdim, double *Q, int64_t plane, const double *y, const CostP &cp, double *vpart,
                             int64_t ldp, hipStream_t st);

}  // namespace plship
