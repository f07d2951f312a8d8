// Launcher of small_rank_step_kernel<KB, COST, LINK, VALUE, PRIOR> for ONE value of VALUE; included by small_rank_step.hip and
// small_rank_step_value.hip (56 kernel instantiations each, compiled in parallel).
#include "common.h"
#include "small_rank_step.h"
#include "small_rank_step_launch.h"

namespace plship {

template <bool VALUE, bool PRIOR, int COST, int LINK>
static int launch_small_rank_step_cl(const SrStepP &p, hipStream_t st) {
  dim3 grid((unsigned)cdiv(p.J, 16), (unsigned)p.nsplit);
  LaunchScope scope(PLS_TAG_SMALL_RANK_STEP, st);
  const int rc = for_rank_blocks("small_rank_step", p.K, [&](auto kb) -> int {
    constexpr int KB = decltype(kb)::value;
    if (int rc = ensure_lds<small_rank_step_kernel<KB, COST, LINK, VALUE, PRIOR>>(srs_lds_bytes<KB>())) return rc;
    hipLaunchKernelGGL((small_rank_step_kernel<KB, COST, LINK, VALUE, PRIOR>), grid, dim3(256), srs_lds_bytes<KB>(), st, p);
    return PLS_OK;
  });
  return rc ? rc : check_launch("small_rank_step");
}

// one instantiation per (cost, link) pair of for_cost_link's list (cost_device.h)
template <bool VALUE, bool PRIOR>
static int launch_small_rank_step_any(const SrStepP &p, hipStream_t st) {
  return for_cost_link(p.cp, [&](auto c, auto l) {
    return launch_small_rank_step_cl<VALUE, PRIOR, decltype(c)::value, decltype(l)::value>(p, st);
  });
}

}  // namespace plship
