"""Small wrappers over libplship's primitive entry points, shared by the prediction-side code."""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L


def gemm_tn(lm: torch.Tensor, rm: torch.Tensor, alpha: float = 1.0, beta: float = 0.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """out (I x J) = alpha * lm^T rm + beta * out with lm (K x I), rm (K x J) row-major device float64 (pls_gemm_tn)."""
    L.require_gpu_tensor(lm, "lm")
    L.require_gpu_tensor(rm, "rm")
    lm = lm if lm.stride(1) == 1 else lm.contiguous()
    rm = rm if rm.stride(1) == 1 else rm.contiguous()
    k, i = lm.shape
    k2, j = rm.shape
    assert k == k2, f"contraction mismatch {lm.shape} vs {rm.shape}"
    if out is None:
        assert beta == 0.0
        out = torch.empty((i, j), dtype=torch.float64, device=lm.device)
    assert out.shape == (i, j) and (out.stride(1) == 1 or j <= 1)
    L.check(
        L.load().pls_gemm_tn(lm.data_ptr(), L.ld(lm), rm.data_ptr(), L.ld(rm), out.data_ptr(), L.ld(out), i, j, k, float(alpha),
                             float(beta), L.stream_ptr()),
        "pls_gemm_tn",
    )
    return out


def sym_eigh(matrix: torch.Tensor, return_info: bool = False):
    """(eigenvalues ascending, eigenvectors as columns) of the symmetric device matrix whose LOWER triangle ``matrix`` holds
    (pls_sym_eigh: libplship's blocked Jacobi solver; the drop-in for torch.linalg.eigh at orthonormal.py:46-48 and
    samplers.py:27 of the reference).  Each eigenvector's largest-magnitude component is positive (canonicalise_signs of
    basis/spectrum.py is the identity on the result).  The call synchronises the stream.  ``return_info``: also the
    solver's info (0 converged, 1 sweep cap reached); without it a result that did not converge warns."""
    a = L.require_gpu_tensor(matrix, "matrix", promote=True)
    assert a.dim() == 2 and a.shape[0] == a.shape[1], f"square matrix expected, got {tuple(a.shape)}"
    a = a if a.stride(1) == 1 else a.contiguous()
    m = a.shape[0]
    lam = torch.empty(m, dtype=torch.float64, device=a.device)
    vec = torch.empty((m, m), dtype=torch.float64, device=a.device)
    info = ctypes.c_int32(0)
    if m:
        lib = L.load()
        nbytes = lib.pls_sym_eigh_workspace_bytes(m)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
        L.check(lib.pls_sym_eigh(a.data_ptr(), L.ld(a), m, lam.data_ptr(), vec.data_ptr(), m, ctypes.byref(info), ws.data_ptr(),
                                 nbytes, L.stream_ptr()), "pls_sym_eigh")
    if return_info:
        return lam, vec, int(info.value)
    if info.value:
        import warnings

        warnings.warn(f"pls_sym_eigh: the sweep cap was reached for a {m} x {m} matrix (info = {info.value}); the result is the "
                      "last iterate")
    return lam, vec


def row_power_sums(s: torch.Tensor, power: int, shift: torch.Tensor | None = None) -> torch.Tensor:
    """(rows,) vector of sum_j (s[r, j] - shift[r])^power (pls_row_power_sums; fixed summation order)."""
    L.require_gpu_tensor(s, "samples")
    s = s if s.stride(1) == 1 else s.contiguous()
    rows, cols = s.shape
    out = torch.empty(rows, dtype=torch.float64, device=s.device)
    sh = None if shift is None else L.require_gpu_tensor(shift, "shift").contiguous()
    L.check(
        L.load().pls_row_power_sums(s.data_ptr(), L.ld(s), rows, cols, L.ptr(sh), int(power), out.data_ptr(), L.stream_ptr()),
        "pls_row_power_sums",
    )
    return out


def row_quantiles(s: torch.Tensor, qs) -> torch.Tensor:
    """(rows, len(qs)) quantiles over dim 1 with torch.quantile's linear interpolation (pls_row_quantiles: one LDS sort per
    row up to 16384 samples, radix selection of the two order statistics beyond -- a calibration split above 16384 points,
    the gathered samples of a J-sharded run)."""
    L.require_gpu_tensor(s, "samples")
    s = s if s.stride(1) == 1 else s.contiguous()
    rows, cols = s.shape
    q = torch.as_tensor(list(qs), dtype=torch.float64).to(s.device)
    out = torch.empty((rows, q.numel()), dtype=torch.float64, device=s.device)
    L.check(
        L.load().pls_row_quantiles(s.data_ptr(), L.ld(s), rows, cols, q.data_ptr(), q.numel(), out.data_ptr(), q.numel(),
                                   L.stream_ptr()),
        "pls_row_quantiles",
    )
    return out


def block_means(e: torch.Tensor, block_cols: int | None = None, out: torch.Tensor | None = None, out_ptr: int | None = None) -> torch.Tensor | None:
    """Means of consecutive blocks of ``block_cols`` entries of the per-particle vector ``e`` (pls_block_means; the whole
    vector when block_cols is None): the ``.mean()`` of orthonormal.py:126 / inducing_point.py:115 as a fixed-order
    libplship reduction.  ``out``: device vector to fill; ``out_ptr``: raw address instead (pinned host memory mapped into
    the device: the value is read on the host after an event, with no copy kernel)."""
    L.require_gpu_tensor(e, "energies")
    e = e.contiguous()
    j = e.numel()
    bc = j if block_cols is None else int(block_cols)
    nb = (j + bc - 1) // bc if j else 0
    if out_ptr is None:
        if out is None:
            out = torch.empty(nb, dtype=torch.float64, device=e.device)
        assert out.numel() >= nb and out.is_contiguous()
        out_ptr = out.data_ptr()
    if j:
        L.check(L.load().pls_block_means(e.data_ptr(), j, max(bc, 1), out_ptr, L.stream_ptr()), "pls_block_means")
    return out
