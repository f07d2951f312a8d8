// Workspace layout of the marginal-likelihood evaluation (gp_mll.hip): shared by its plan and the workspace formulas of
// pls_gp_mll_grad.  The geometry of the pairwise kernels it calls is base_kernel.h.
#pragma once
#include <stdint.h>

namespace plship {

// leading dimension of the n x n planes of pls_gp_mll_grad: n rounded up to even (16-byte rows)
static inline int64_t gp_mll_ld(int64_t n) { return (n + 1) & ~(int64_t)1; }
// doubles of a vector of n entries, rounded up so that what follows stays 16-byte aligned
static inline int64_t gp_mll_vec(int64_t n) { return (n + 1) & ~(int64_t)1; }

}  // namespace plship
