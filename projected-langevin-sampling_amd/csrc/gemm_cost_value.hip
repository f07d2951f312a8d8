// libplship.so: the forward GEMM with the cost-VALUE epilogue (stand-alone energy), one instantiation per (cost, link)
// pair the reference's experiments use plus the run-time switch.
#include "common.h"
#include "cost_epilogues.h"
#include "gemm_launch.h"

namespace plship {

// (one instantiation per pair of for_cost_link's list, cost_device.h; the tile geometry is part of the epilogue type)
int launch_cost_value_gemm(const double *Lf, int64_t ldlf, const double *V, int64_t ldv, int64_t rows, int64_t j, int64_t kdim,
                           double *partial, int64_t ldp, const double *y, const CostP &cp, hipStream_t st) {
  return for_cost_link(cp, [&](auto c, auto l) {
    constexpr int COST = decltype(c)::value, LINK = decltype(l)::value;
    GemmShape g{Lf, ldlf, V, ldv, rows, j, kdim, 0, 0, 0};
    if (use_big_tiles(rows, j)) {
      EpiCostValue<128, 128, 64, 64, COST, LINK> e{partial, ldp, y, cp};
      return launch_gemm_cfg<128, 128, 64, 64>(g, e, st);
    }
    EpiCostValue<64, 64, 32, 32, COST, LINK> e{partial, ldp, y, cp};
    return launch_gemm_cfg<64, 64, 32, 32>(g, e, st);
  });
}

}  // namespace plship
