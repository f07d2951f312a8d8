// libplship.so: the forward GEMM with the cost-derivative epilogues, one instantiation per (cost, link) pair the
// reference's experiments use plus the run-time switch (its own translation unit: 14 GEMM kernels).
#include "common.h"
#include "cost_epilogues.h"
#include "gemm_launch.h"
#include "winograd.h"

namespace plship {

// (one instantiation per pair of for_cost_link's list, cost_device.h; Gaussian/identity has epilogues of its own that go
// from the registers straight to global memory)
int launch_cost_deriv_gemm(const double *Lf, int64_t ldlf, const double *V, int64_t ldv, int64_t rows, int64_t j, int64_t kdim,
                           double *G, int64_t ldg, const double *y, const CostP &cp, double *vpart, int64_t ldp,
                           hipStream_t st) {
  return for_cost_link(cp, [&](auto c, auto l) {
    constexpr int COST = decltype(c)::value, LINK = decltype(l)::value;
    if constexpr (COST == PLS_COST_GAUSSIAN && LINK == PLS_LINK_IDENTITY) {
      EpiGaussDeriv e{G, ldg, y, 1.0 / cp.p0, vpart, ldp};
      return launch_gemm(Lf, ldlf, V, ldv, rows, j, kdim, e, st);
    } else {
      EpiCostDeriv<COST, LINK> e{G, ldg, y, cp, vpart, ldp};
      return launch_gemm(Lf, ldlf, V, ldv, rows, j, kdim, e, st);
    }
  });
}

int launch_cost_deriv_paired(const double *Lf, int64_t ldlf, int64_t pair_i, const double *V, int64_t ldv, int64_t pair_j,
                             int64_t rows, int64_t kdim, double *Q, int64_t plane, const double *y, const CostP &cp, double *vpart,
                             int64_t ldp, hipStream_t st) {
  return for_cost_link(cp, [&](auto c, auto l) {
    constexpr int COST = decltype(c)::value, LINK = decltype(l)::value;
    if constexpr (COST == PLS_COST_GAUSSIAN && LINK == PLS_LINK_IDENTITY) {
      EpiWinoGauss e{Q, pair_j, plane, y, pair_i, pair_j, 1.0 / cp.p0, vpart, ldp};
      return launch_gemm_paired(Lf, ldlf, pair_i, V, ldv, pair_j, rows, kdim, e, st);
    } else {
      EpiWinoCost<COST, LINK> e{Q, pair_j, plane, y, pair_i, pair_j, cp, vpart, ldp};
      return launch_gemm_paired(Lf, ldlf, pair_i, V, ldv, pair_j, rows, kdim, e, st);
    }
  });
}

}  // namespace plship
