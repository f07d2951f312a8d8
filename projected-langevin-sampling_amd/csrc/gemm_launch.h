// GEMM launch helpers shared by the translation units that instantiate gemm_tn_f64_kernel.
#pragma once
#include "common.h"
#include "gemm_tn_f64.h"

namespace plship {

#ifdef PLS_STAMP
extern unsigned long long *g_stamp_buffer;  // diagnostic build only (tools/stamp_probe.py); defined in plship.hip
#endif

// ---------------------------------------------------------------------------------------------------------------
// GEMM launcher
// ---------------------------------------------------------------------------------------------------------------
// Every launcher of a configuration whose k-loop copies by LDS-DMA (the 128 x 128 tiles, their row-block, paired and
// Winograd-product forms) calls this first, before anything touches the device: operands of lcols / rcols columns whose
// leading dimension the DMA's 32-bit offsets cannot address (gemm_dma_max_ld) are refused, not contracted with zeros.
// Operands that are not 16-byte aligned with even leading dimensions go through registers with 64-bit addresses: no limit.
static inline int gemm_dma_check(const double *L, int64_t ldl, int64_t lcols, const double *R, int64_t ldr, int64_t rcols) {
  if (!gemm_vec_operands(L, ldl, R, ldr)) return PLS_OK;
  if (ldl > gemm_dma_max_ld(lcols))
    return fail(PLS_ERR_INVALID_ARGUMENT, "gemm: leading dimension ldl=%lld of the %lld-column left operand is beyond %lld, the "
                "largest the 128 x 128 tiles address", (long long)ldl, (long long)lcols, (long long)gemm_dma_max_ld(lcols));
  if (ldr > gemm_dma_max_ld(rcols))
    return fail(PLS_ERR_INVALID_ARGUMENT, "gemm: leading dimension ldr=%lld of the %lld-column right operand is beyond %lld, the "
                "largest the 128 x 128 tiles address", (long long)ldr, (long long)rcols, (long long)gemm_dma_max_ld(rcols));
  return PLS_OK;
}

template <int BI, int BJ, int WI, int WJ, class Epi, int MINW = ((BI >= 128) ? 2 : 4)>
static int launch_gemm_cfg(GemmShape g, const Epi &epi, hipStream_t st) {
  constexpr int BK = 16;  // MINW: waves per SIMD the register allocation must leave room for
  constexpr int NT = (BI / WI) * (BJ / WJ) * 64;
  constexpr size_t lds_bytes = gemm_tile_lds_bytes(BI, BJ, BK);
  constexpr auto kern = gemm_tn_f64_kernel<BI, BJ, WI, WJ, BK, MINW, Epi>;
  if constexpr (BI == 128 && BJ == 128)  // (gemm_tile's kDma)
    if (int rc = gemm_dma_check(g.L, g.ldl, g.I, g.R, g.ldr, g.J)) return rc;
  if (int rc = ensure_lds<kern>(lds_bytes)) return rc;
#ifdef PLS_STAMP
  g.stamps = g_stamp_buffer;
  // diagnostic build only: PLS_STAMP_LDS_PAD=<bytes> of extra dynamic LDS (e.g. 90000: one workgroup per CU)
  static const size_t pad = getenv("PLS_STAMP_LDS_PAD") ? (size_t)atol(getenv("PLS_STAMP_LDS_PAD")) : 0;
  if (pad)
    if (int rc = ensure_lds<kern, 1>(lds_bytes + pad)) return rc;
  const size_t lds_launch = lds_bytes + pad;
#else
  const size_t lds_launch = lds_bytes;
#endif
  g.nti = (int)cdiv(g.I, BI);
  g.ntj = (int)cdiv(g.J, BJ);
  // (a triangular operand pairs tile rows t and nti - 1 - t in one workgroup: gemm_tn_f64_kernel)
  const int64_t nwg = (int64_t)((g.tri && Epi::kTag == 1) ? (g.nti + 1) / 2 : g.nti) * g.ntj;
  if (nwg <= 0) return PLS_OK;
  if (nwg > 0x7fffffff) return fail(PLS_ERR_INVALID_ARGUMENT, "gemm: too many tiles");
  unsigned nsplit = 1;
  if (g.kchunk > 0 && g.kchunk < g.K) nsplit = (unsigned)cdiv(g.K, g.kchunk);
  {
    LaunchScope scope(Epi::kTag, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg, nsplit), dim3(NT), lds_launch, st, g, epi);
  }
  return check_launch("gemm_tn_f64");
}

static inline bool use_big_tiles(int64_t I, int64_t J, int64_t nsplit = 1) { return cdiv(I, 128) * cdiv(J, 128) * nsplit >= 256; }

// kchunk > 0 (EpiStore only): split-K into cdiv(K, kchunk) slabs, one grid.y plane each
template <class Epi>
static int launch_gemm(const double *L, int64_t ldl, const double *R, int64_t ldr, int64_t I, int64_t J, int64_t K,
                       const Epi &epi, hipStream_t st, int64_t kchunk = 0, int tri = 0) {
  GemmShape g{L, ldl, R, ldr, I, J, K, 0, 0, kchunk, tri};
  const int64_t nsplit = (kchunk > 0 && kchunk < K) ? cdiv(K, kchunk) : 1;
  if (use_big_tiles(I, J, nsplit)) return launch_gemm_cfg<128, 128, 64, 64>(g, epi, st);
  return launch_gemm_cfg<64, 64, 32, 32>(g, epi, st);
}

}  // namespace plship
