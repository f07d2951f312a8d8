// Launcher of small_rank_kernel<KB, MODE, COST, LINK> for ONE mode; included by small_rank_{drift,value,drift_value}.hip
// (one translation unit per mode: 56 kernel instantiations each, compiled in parallel).
#include "common.h"
#include "small_rank.h"
#include "small_rank_launch.h"

namespace plship {

template <int MODE, int COST, int LINK>
static int launch_small_rank_cl(const SmallRankP &p, int64_t nsplit, hipStream_t st) {
  dim3 grid((unsigned)cdiv(p.J, 64), (unsigned)nsplit);
  LaunchScope scope(MODE == SR_MODE_VALUE ? PLS_TAG_SMALL_RANK_VALUE : PLS_TAG_SMALL_RANK_DRIFT, st);
  const int rc = for_rank_blocks("small_rank", p.K, [&](auto kb) -> int {
    constexpr int KB = decltype(kb)::value;
    if (int rc = ensure_lds<small_rank_kernel<KB, MODE, COST, LINK>>(sr_lds_bytes<KB>())) return rc;
    hipLaunchKernelGGL((small_rank_kernel<KB, MODE, COST, LINK>), grid, dim3(256), sr_lds_bytes<KB>(), st, p);
    return PLS_OK;
  });
  return rc ? rc : check_launch("small_rank");
}

// one instantiation per (cost, link) pair of for_cost_link's list (cost_device.h)
template <int MODE>
static int launch_small_rank(const SmallRankP &p, int64_t nsplit, hipStream_t st) {
  return for_cost_link(p.cp, [&](auto c, auto l) {
    return launch_small_rank_cl<MODE, decltype(c)::value, decltype(l)::value>(p, nsplit, st);
  });
}

}  // namespace plship
