// Geometry of the marginal-likelihood gradient reduction and of the fused predictive mean (gp_mll.hip): shared by the
// kernels, their launchers and the workspace formulas of pls_kernel_grad_sums / pls_gp_mll_grad.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace plship {

constexpr int GRAD_ROWS = 64;    // rows of a workgroup's tile (as GRAM_ROWS of the Gram build)
constexpr int GRAD_COLS = 512;   // columns of a workgroup's tile: 256 threads, a pair of columns each
constexpr int GRAD_D_MAX = 64;   // largest input dimension

// pls_kernel_mean: test points of a workgroup (one per lane, the four waves split the training points), and the training
// points staged in LDS at a time: 32 KiB of pre-scaled coordinates, 512 points at the most; a multiple of 4 for every D_MAX
constexpr int MEAN_POINTS = 64;
constexpr int mean_chunk(int d_max) { return 4096 / d_max < 512 ? 4096 / d_max : 512; }

// workgroups of the reduction over an n x n matrix = partial rows of d + 1 doubles in its workspace
static inline int64_t grad_sums_blocks(int64_t n) { return cdiv(n, GRAD_COLS) * cdiv(n, GRAD_ROWS); }
// leading dimension of the n x n planes of pls_gp_mll_grad: n rounded up to even (16-byte rows)
static inline int64_t gp_mll_ld(int64_t n) { return (n + 1) & ~(int64_t)1; }
// doubles of a vector of n entries, rounded up so that what follows stays 16-byte aligned
static inline int64_t gp_mll_vec(int64_t n) { return (n + 1) & ~(int64_t)1; }

}  // namespace plship
