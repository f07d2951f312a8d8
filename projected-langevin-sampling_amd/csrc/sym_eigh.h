// Geometry of the symmetric eigensolver (sym_eigh.hip): block sizes, sweep caps, the round-robin schedule shared by the
// kernels and pls_sym_eigh_round_pairs, and the workspace layout of pls_sym_eigh.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace plship {

constexpr int EIGH_SUB = 64;           // largest problem one workgroup diagonalises in LDS; edge of a tile
constexpr int EIGH_BLOCK = 32;         // block edge for m > EIGH_SUB (a pair of blocks is one EIGH_SUB problem)
constexpr int EIGH_LD = EIGH_SUB + 1;  // LDS row pitch: rows and columns of a tile both walk distinct banks
constexpr int EIGH_INNER_SWEEPS = 30;  // cap of the sweeps inside jacobi_block_kernel
constexpr int EIGH_OUTER_SWEEPS = 30;  // cap of the sweeps over block pairs
constexpr int EIGH_JACOBI_THREADS = 512;
constexpr int EIGH_TILE_THREADS = 256;

// Tournament (circle) schedule.  `players` is even; round r in [0, players - 1) seats player players - 1 against r and
// (r + k) against (r - k) mod (players - 1) for k = 1 .. players / 2 - 1: players / 2 disjoint pairs per round, every
// unordered pair exactly once per players - 1 rounds (x + y = 2 r has one solution r modulo the odd players - 1).
__host__ __device__ inline void round_robin_pair(int players, int round, int k, int *lo, int *hi) {
  const int m1 = players - 1;
  const int x = k == 0 ? m1 : (round + k) % m1;
  const int y = k == 0 ? round % m1 : (round - k + m1) % m1;
  *lo = x < y ? x : y;
  *hi = x < y ? y : x;
}

// an odd number of blocks plays with one dummy: whoever meets it has a bye
__host__ __device__ inline int eigh_players(int64_t nblocks) { return (int)(nblocks + (nblocks & 1)); }

struct EighLayout {  // offsets in doubles into the workspace
  int64_t mp = 0;    // padded order: m rounded up to EIGH_BLOCK (EIGH_SUB for the single-launch sizes)
  int64_t nb = 0;    // blocks (0: single launch)
  int64_t w = 0, v = 0, q = 0, stats = 0, counters = 0, total = 0;
};

static inline EighLayout eigh_layout(int64_t m) {
  EighLayout l;
  if (m <= 0) return l;
  const bool blocked = m > EIGH_SUB;
  l.mp = blocked ? cdiv(m, EIGH_BLOCK) * EIGH_BLOCK : EIGH_SUB;
  l.nb = blocked ? l.mp / EIGH_BLOCK : 0;
  const int64_t pairs = blocked ? eigh_players(l.nb) / 2 : 0;
  l.w = 0;                                                   // working matrix (blocked) / the diagonal (single launch)
  l.v = l.w + (blocked ? l.mp * l.mp : (int64_t)EIGH_SUB);   // accumulated rotations
  l.q = l.v + l.mp * l.mp;                                   // one EIGH_SUB x EIGH_SUB rotation per pair of a round
  l.stats = l.q + pairs * EIGH_SUB * EIGH_SUB;               // max |a|, sum (a / max)^2, non-finite flag, spare
  l.counters = l.stats + 4;                                  // int32: rotations per outer sweep, then "not converged"
  l.total = l.counters + (EIGH_OUTER_SWEEPS + 2) / 2;
  return l;
}

}  // namespace plship
