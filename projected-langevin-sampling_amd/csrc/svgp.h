// Geometry of the SVGP minibatch evaluation (svgp.hip): shared by the kernels, their launchers and the workspace formula
// of pls_svgp_workspace_bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace plship {

constexpr int SVGP_TILE = 32;    // points of a workgroup's tile (two 16-row MFMA tiles)
constexpr int SVGP_M_MAX = 256;  // largest number of inducing points (the reference's largest is 191)
constexpr int SVGP_LDS_PAD = 4;  // doubles between the rows of the LDS images: 16 rows x 4 k land on 64 distinct 8-byte slots

// M rounded up to the MFMA tile
static inline int64_t svgp_mp(int64_t m) { return (m + 15) / 16 * 16; }
static inline int64_t svgp_tiles(int64_t b) { return cdiv(b, SVGP_TILE); }
// LDS of a workgroup: the gathered rows and their w images, m, and 7 per-point vectors + a scratch line
static inline size_t svgp_lds_bytes(int64_t mp) {
  return sizeof(double) * (size_t)(2 * SVGP_TILE * (mp + SVGP_LDS_PAD) + mp + 7 * SVGP_TILE + 16);
}
// doubles of one call's workspace: 4 (KL pieces) + 4 per tile (scalar partials) [+ MP (MP + 1) per tile with gradients]
static inline size_t svgp_ws_doubles(int64_t tiles, int64_t mp, bool grad) {
  return (size_t)4 + (size_t)4 * (size_t)tiles + (grad ? (size_t)tiles * (size_t)mp * (size_t)(mp + 1) : (size_t)0);
}

}  // namespace plship
