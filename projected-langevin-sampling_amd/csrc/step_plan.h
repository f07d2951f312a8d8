// Workspace plans of the step and energy entries (plship.hip): the regions a call carves out of the caller's workspace, the
// offset of each (256-byte aligned) and the bytes of the whole.  The size queries (pls_*_workspace_bytes) and the entries
// that carve their workspace up read the same layouts, so a query cannot promise fewer bytes than its entry takes.
// Host-only integer arithmetic: no HIP calls, no allocation; route options come in as arguments.  (The row splits of the fused
// kernels stay next to those kernels, in small_rank.h and small_rank_step.h; the layouts here build on them.)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#ifdef PLS_SRS_PROBE
#include <cstdlib>
#endif

#include "common.h"
#include "small_rank.h"       // small_rank_splits: row slabs of the fused drift / cost kernels
#include "small_rank_step.h"  // small_rank_step_splits, small_rank_step_sync_words: the one-launch step's plan

namespace plship {

static inline size_t mj_bytes(int64_t m, int64_t j) { return align_up((size_t)m * j * sizeof(double), 256); }

// Split-K plan for the back-projection D (I x J) = L^T R with a long contraction (K = rows of the N chunk).  Two reasons
// to cut the contraction into slabs (summed in a fixed order by the update kernel: deterministic, no atomics):
//   occupancy -- too few 128x128 output tiles to put two workgroups on each of the 256 CUs (narrow particle shards);
//   locality  -- over a very long k-loop the co-resident workgroups drift apart and stop sharing operand panels in
//                their XCD's L2: at K = 1e5 one slab reads 66 GB through the fabric, 8 slabs 20 GB, at equal speed
//                (DESIGN.md "tuning log"); slabs of <= 16384 rows keep the drift inside the L2 window.
// Returns the number of slabs (<= 16).
static inline int64_t plan_split_k(int64_t I, int64_t J, int64_t K, int64_t *kchunk) {
  const int64_t tiles = cdiv(I, 128) * cdiv(J, 128);
  int64_t s = 1;
  if (tiles < 512) s = cdiv(512, tiles);
  const int64_t s_local = cdiv(K, 16384);
  if (s_local > s) s = s_local;
  if (s > 16) s = 16;
  // wave quantisation: tiles * s workgroups run in rounds of 512 (2 per CU); a few more slabs can fill the last round
  // (J = 2048: 128 tiles x 7 slabs = 1.75 rounds -> 87 % of the MFMA rate; x 8 = 2 rounds)
  if (s > 1) {
    auto waste = [&](int64_t sl) {
      const double rounds = (double)(tiles * sl) / 512.0;
      return std::ceil(rounds) / rounds;
    };
    int64_t best = s;
    for (int64_t sl = s + 1; sl <= 16 && sl <= s + 4; ++sl)
      if (waste(sl) < waste(best) - 0.03) best = sl;
    s = best;
  }
  // keep every slab's k-loop long enough to amortise its prologue / epilogue; a handful of tiles (small ranks AND few
  // particles) is latency-bound on its serial k-loop instead, so shorter slabs pay (M_k = 129, J = 256, N = 2000:
  // 12 workgroups walked 125 k-steps each)
  const int64_t min_chunk = tiles < 64 ? 256 : 1024;
  while (s > 1 && K / s < min_chunk) --s;
  int64_t kc = cdiv(cdiv(K, s), 16) * 16;
  s = cdiv(K, kc);
  *kchunk = (s > 1) ? kc : 0;
  return s;
}

// D slabs of the general route: the split-K plan, or the fused small-rank kernels' row slabs (sized independently of the
// options)
static inline int64_t onb_max_slabs(int64_t mk, int64_t j, int64_t n) {
  int64_t kc;
  int64_t s = plan_split_k(mk, j, n, &kc);
  if (mk <= 256) {
    int64_t rows;
    const int64_t sr = small_rank_splits(j, n, &rows);
    if (sr > s) s = sr;
  }
  return s;
}

// partial rows of the step's energy by-product: one per 32 data rows of a chunk (the 64x64-tile worst case), or one per
// small-rank row slab (<= 32); sized for the chunk, not for N
static inline int64_t energy_partial_rows(int64_t n_chunk) { return cdiv(n_chunk, 32) < 32 ? 32 : cdiv(n_chunk, 32); }
static inline size_t onb_energy_partial_bytes(int64_t n_chunk, int64_t j) {
  return align_up((size_t)energy_partial_rows(n_chunk) * j * sizeof(double), 256);
}

// Partial rows of the Gaussian/identity fast path's energy (fast_step_launch, fast_energy_launch): one per 64 operator rows
// with the 64 x 64 tiles; one per 128 rows with the 128 x 128 tiles, two in the step's epilogue.  2 cdiv(mk, 128) rows hold
// every tiling of the step (pls_energy_partials_bytes, pls_ipb_whitened_workspace_bytes).
static inline int64_t gaussian_partial_rows(int64_t mk, bool big_tiles, bool step) {
  return big_tiles ? (step ? 2 : 1) * cdiv(mk, 128) : cdiv(mk, 64);
}
static inline size_t gaussian_partial_bytes(int64_t rows, int64_t j) { return (size_t)rows * j * sizeof(double); }
static inline size_t gaussian_step_partial_bytes(int64_t mk, int64_t j) { return gaussian_partial_bytes(gaussian_partial_rows(mk, true, true), j); }

// ---- the one-launch small-rank step (small_rank_step.h) ---------------------------------------------------------------
// [lead m x j buffers][slabs: partial drifts + cost sums, cdiv(j, 16) x ns x (mk + 1) x 16 doubles, none with one slab]
// [arrival counters: when the slabs or the energy sums need them and the caller brings none (pls_block_desc.step_sync)]
struct SrStepLayout {
  int64_t ns, rows;  // slabs per column block, rows per slab
  size_t slab_off, slab_bytes;
  bool counters;
  size_t sync_off, sync_bytes;
  size_t total;
};

static inline SrStepLayout sr_step_layout(int lead, int64_t mk, int64_t n, int64_t j, bool sums, bool own_sync) {
  SrStepLayout L{};
  L.ns = small_rank_step_splits(j, n, (int)mk, &L.rows);
#ifdef PLS_SRS_PROBE
  if (const char *f = getenv("PLS_SRS_FORCE_NS")) {
    L.ns = atoi(f);
    L.rows = (cdiv(n, L.ns) + 63) / 64 * 64;
    L.ns = cdiv(n, L.rows);
  }
#endif
  L.slab_off = (size_t)lead * mj_bytes(mk, j);
  L.slab_bytes = L.ns > 1 ? align_up((size_t)cdiv(j, 16) * L.ns * ((size_t)mk + 1) * 16 * sizeof(double), 256) : 0;
  L.counters = (L.ns > 1 || sums) && !own_sync;
  L.sync_off = L.slab_off + L.slab_bytes;
  L.sync_bytes = small_rank_step_sync_words(j) * sizeof(uint32_t);
  L.total = L.sync_off + (L.counters ? align_up(L.sync_bytes, 256) : 0);
  return L;
}

// what a size query promises the one-launch step: counters included; 0 where the step does not apply (mk outside 1..128)
static inline size_t sr_step_query_bytes(int lead, int64_t mk, int64_t n, int64_t j) {
  return (mk < 1 || mk > 128) ? 0 : sr_step_layout(lead, mk, n, j, true, false).total;
}

// ---- the general route (stream_drift) -----------------------------------------------------------------------------------
// [lead m x j buffers: none on the orthonormal basis, V, xi, e on the inducing-point basis][D slabs, m x j each]
// [partial rows of the energy by-product][G chunk, n_chunk x j]
struct DriftLayout {
  size_t mj;                    // one m x j buffer; lead buffer i at i * mj
  int64_t slabs;                // D slabs
  int64_t n_chunk, part_rows;   // data rows per chunk, partial rows of the energy by-product
  size_t d_off, part_off, g_off, total;
};

// the chunk-dependent regions of a layout: the partial rows and the G chunk
static inline DriftLayout drift_chunk(DriftLayout L, int64_t j, int64_t n_chunk) {
  L.n_chunk = n_chunk;
  L.part_rows = energy_partial_rows(n_chunk);
  L.g_off = L.part_off + onb_energy_partial_bytes(n_chunk, j);
  L.total = L.g_off + (size_t)n_chunk * j * sizeof(double);
  return L;
}

static inline DriftLayout drift_layout(int lead, int64_t mk, int64_t n, int64_t j, int64_t n_chunk) {
  DriftLayout L{};
  L.mj = mj_bytes(mk, j);
  L.slabs = onb_max_slabs(mk, j, n);
  L.d_off = (size_t)lead * L.mj;
  L.part_off = L.d_off + (size_t)L.slabs * L.mj;
  return drift_chunk(L, j, n_chunk);
}

// The layout of the largest chunk that fits `avail` bytes: all n rows, else a multiple of 128, never below min(n, 128).
// When not even min(n, 128) rows fit, that layout all the same: its total exceeds `avail`, and the caller reports it.
static inline DriftLayout drift_plan(int lead, int64_t mk, int64_t n, int64_t j, size_t avail) {
  const DriftLayout all = drift_layout(lead, mk, n, j, n);
  if (all.total <= avail) return all;
  auto fits = [&](int64_t c) { return drift_chunk(all, j, c).total <= avail; };
  const int64_t min_rows = n < 128 ? n : 128;
  if (!fits(min_rows)) return drift_chunk(all, j, min_rows);
  // start from the estimate the per-row bytes give, then walk to the largest multiple of 128 that fits
  const size_t left = avail - all.part_off;
  const double per_row = (double)j * sizeof(double) * (1.0 + 1.0 / 32.0);
  int64_t c = (int64_t)(((double)left - 32.0 * j * sizeof(double) - 512.0) / per_row);
  if (c > n) c = n;
  c = c / 128 * 128;
  while (c > min_rows && !fits(c)) c -= 128;
  while (c + 128 <= n && fits(c + 128)) c += 128;
  return drift_chunk(all, j, c < min_rows ? min_rows : c);
}

// ---- the Winograd route of the orthonormal basis (winograd.h) --------------------------------------------------------------
// [the seven products' D slabs, M_k/2 x J/2 each, product-major][partial rows of the energy by-product][the seven right-hand
// planes of a chunk, n_chunk x J/2 each].  Chunks are ranges of PAIRED rows (row p stands for data rows p and p + N/2).  The
// left-hand planes S1..S4 (N/2 x M_k/2 each, s_plane bytes apart) are the basis' own (pls_onb_winograd_prepare), not workspace.
struct WinoLayout {
  int64_t mh, nh, jh;          // M_k / 2, N / 2, J / 2
  int64_t slabs;               // split-K slabs of each product
  int64_t n_chunk, part_rows;  // paired rows per chunk, partial rows of the energy by-product
  size_t s_plane, p_slab, q_plane;  // bytes of one left-hand plane, one product slab, one right-hand plane
  size_t p_off, part_off, q_off, total;
};

// Split-K plan of the seven products (M_k/2 x J/2 each) over K paired rows: the slabs that put the 7 x tiles x slabs
// workgroups in whole rounds of 512 (2 per CU), with slabs of <= 16384 rows (the L2 locality of plan_split_k).  <= 16.
static inline int64_t wino_split_k(int64_t mh, int64_t jh, int64_t K, int64_t *kchunk) {
  const int64_t tiles = 7 * cdiv(mh, 128) * cdiv(jh, 128);
  int64_t s = tiles < 512 ? cdiv(512, tiles) : 1;
  const int64_t s_local = cdiv(K, 16384);
  if (s_local > s) s = s_local;
  if (s > 16) s = 16;
  auto waste = [&](int64_t sl) {
    const double rounds = (double)(tiles * sl) / 512.0;
    return std::ceil(rounds) / rounds;
  };
  int64_t best = s;
  for (int64_t sl = s + 1; sl <= 16 && sl <= s + 4; ++sl)
    if (waste(sl) < waste(best) - 0.03) best = sl;
  s = best;
  while (s > 1 && K / s < 1024) --s;
  int64_t kc = cdiv(cdiv(K, s), 16) * 16;
  s = cdiv(K, kc);
  *kchunk = (s > 1) ? kc : 0;
  return s;
}

// one left-hand plane (N/2 x M_k/2); the four take 4 x this
static inline size_t wino_left_plane_bytes(int64_t mk, int64_t n) { return align_up((size_t)(n / 2) * (mk / 2) * sizeof(double), 256); }

static inline WinoLayout wino_chunk(WinoLayout L, int64_t n_chunk) {
  L.n_chunk = n_chunk;
  L.part_rows = energy_partial_rows(n_chunk);
  L.q_plane = align_up((size_t)n_chunk * L.jh * sizeof(double), 256);
  L.q_off = L.part_off + align_up((size_t)L.part_rows * 2 * L.jh * sizeof(double), 256);
  L.total = L.q_off + 7 * L.q_plane;
  return L;
}

// the layout for chunks of n_chunk paired rows; the slab count is planned for the largest chunk
static inline WinoLayout wino_layout(int64_t mk, int64_t n, int64_t j, int64_t n_chunk) {
  WinoLayout L{};
  L.mh = mk / 2;
  L.nh = n / 2;
  L.jh = j / 2;
  int64_t kc;
  L.slabs = wino_split_k(L.mh, L.jh, n_chunk < L.nh ? n_chunk : L.nh, &kc);
  L.s_plane = wino_left_plane_bytes(mk, n);
  L.p_slab = align_up((size_t)L.mh * L.jh * sizeof(double), 256);
  L.p_off = 0;
  L.part_off = L.p_off + 7 * (size_t)L.slabs * L.p_slab;
  return wino_chunk(L, n_chunk);
}

// The layout of the largest chunk that fits `avail` bytes: all N/2 paired rows, else a multiple of 128, never below
// min(N/2, 128); when not even that fits, that layout all the same (its total exceeds `avail`: the caller takes another route)
static inline WinoLayout wino_plan(int64_t mk, int64_t n, int64_t j, size_t avail) {
  const int64_t nh = n / 2;
  const WinoLayout all = wino_layout(mk, n, j, nh);
  if (all.total <= avail) return all;
  const int64_t min_rows = nh < 128 ? nh : 128;
  int64_t c = nh / 128 * 128;
  while (c > min_rows && wino_layout(mk, n, j, c).total > avail) c -= 128;
  return wino_layout(mk, n, j, c < min_rows ? min_rows : c);
}

// ---- the energy entries (pls_onb_energy, pls_ipb_energy) ---------------------------------------------------------------
// [lead m x j buffers: none on the orthonormal basis, V on the inducing-point basis][partial rows].  The cost value streams N
// in chunks and leaves one partial row per 64 data rows of a chunk, at least two.  The Gaussian/identity fast path reduces
// its quadratic form over M_k instead: at most cdiv(mk, 64) partial rows -- on the inducing-point basis in a second m x j
// buffer, which first holds B V.
struct EnergyLayout {
  size_t part_off;     // the partial rows of the cost value
  int64_t part_rows;   // of the cost value
  int64_t n_chunk;     // data rows per chunk of the cost value
  size_t gauss_bytes;  // what the Gaussian/identity fast path takes from the start of the workspace
  size_t total;
};

static inline EnergyLayout energy_layout(int lead, int64_t mk, int64_t j, int64_t n_chunk) {
  EnergyLayout L{};
  L.part_off = (size_t)lead * mj_bytes(mk, j);
  L.n_chunk = n_chunk;
  L.part_rows = cdiv(n_chunk, 64) < 2 ? 2 : cdiv(n_chunk, 64);
  L.gauss_bytes = lead ? L.part_off + mj_bytes(mk, j) : gaussian_partial_bytes(gaussian_partial_rows(mk, false, false), j);
  const size_t generic = L.part_off + (size_t)L.part_rows * j * sizeof(double);
  L.total = generic > L.gauss_bytes ? generic : L.gauss_bytes;
  return L;
}

// The cost value's chunk that `avail` bytes hold: as many partial rows as fit, their 64 data rows each for the chunk -- all n
// rows, else a multiple of 128.  part_rows < 2: too small.
static inline EnergyLayout energy_plan(int lead, int64_t mk, int64_t n, int64_t j, size_t avail) {
  EnergyLayout L = energy_layout(lead, mk, j, 0);
  L.part_rows = avail > L.part_off ? (int64_t)((avail - L.part_off) / ((size_t)j * sizeof(double))) : 0;
  L.n_chunk = L.part_rows * 64 > n ? n : L.part_rows * 64 / 128 * 128;
  L.total = L.part_off + (size_t)L.part_rows * j * sizeof(double);
  return L;
}

}  // namespace plship
