"""Helpers of tests/test_gpu_large_ld.py and tests/test_large_ld_host.py: operands with leading dimensions at the limits of
the kernels' 32-bit byte offsets (profiles/large_ld_limits.txt), each a view into an arena of one sentinel bit pattern.

Several buffer descriptors of the kernels span 2 GiB whatever the operand's size, so a wrong but in-range offset lands
BEHIND the operand.  An arena therefore starts 16-byte aligned (torch's allocator), reaches at least 2 GiB past the view's
first byte (or to the view's own end, if that is further) and is filled with SENTINEL -- a NaN with a payload no kernel
produces -- before the view's live elements are written.  After the call ``Arena.check`` holds every element outside the live
ones to the sentinel and the live ones to what the caller expects, bit for bit: a stray store shows up, and stays inside our
own allocation."""
import ctypes

import torch

SENTINEL = 0x7FF85EED0BADF00D  # a quiet NaN with a payload
GIB2 = 2 ** 31 // 8  # doubles in 2 GiB
CAP_BYTES = 12 * 2 ** 30  # what one test may hold on the device

# the limits of profiles/large_ld_limits.txt, as formulas; tests/test_large_ld_host.py holds the library's pls_ld_limit to them
DMA_RANGE = 0x7FFFFFF0
STRIP_RANGE = 0x7FFFFF00
DIRECT_MAX_LD = 2 ** 21  # first leading dimension whose tiles leave through LDS
KSPLIT_MAX_LD = 2 ** 22  # first leading dimension handed to the tile kernels
SMALL_RANK_MAX_LD = 2 ** 23  # last leading dimension the fused small-rank kernels take


def gemm_dma_max_ld(cols):
    """128 x 128 tiles, LDS-DMA k-loop: (15 ld + cols) * 8 <= DMA_RANGE, an odd cols rounded up (the lanes load column pairs)"""
    return (DMA_RANGE - 8 * (cols + cols % 2)) // 120


def strip_max_ld(m, cols):
    """substitution kernel: ((min(m, 128) - 1) ld + cols) * 8 <= STRIP_RANGE"""
    rows = min(m, 128)
    return (STRIP_RANGE // 8 - cols) // (rows - 1)


def ipb_prep_max_ld(m):
    """solve-and-noise launch: ((m - 1) ld + m) * 8 <= DMA_RANGE"""
    return (DMA_RANGE // 8 - m) // (m - 1)


class Arena:
    """A (rows, cols) view with leading dimension ``ld`` whose first element sits ``lead`` doubles into a sentinel arena
    (``lead`` odd: the view is 8 bytes off a 16-byte boundary)."""

    def __init__(self, rows, cols, ld, lead=0, values=None):
        assert ld >= cols
        span = (rows - 1) * ld + cols
        self.n = lead + max(span, GIB2)
        self.buf = torch.empty(self.n, dtype=torch.float64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.bits = self.buf.view(torch.int64)
        self.bits.fill_(SENTINEL)
        self.view = self.buf.as_strided((rows, cols), (ld, 1), lead)
        self.ld, self.rows, self.cols = ld, rows, cols
        self.values = None
        if values is not None:
            self.values = values
            self.view.copy_(values)

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def nbytes(self):
        return self.n * 8

    def check(self, want=None, what=""):
        """The live elements equal ``want`` (default: what was written, an input) bit for bit -- or are all still the
        sentinel with ``want="untouched"`` -- and everything else in the arena is the sentinel."""
        live = self.bits.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset())
        if isinstance(want, str):
            assert want == "untouched"
            assert bool((live == SENTINEL).all()), f"{what}: a refused call wrote its output"
        else:
            want = self.values if want is None else want
            got = self.view.cpu()
            bad = (got.view(torch.int64) != want.contiguous().view(torch.int64))
            assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at " \
                                  f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()!r}, want {want[bad][0].item()!r}"
        live.fill_(SENTINEL)
        touched = 0
        for c0 in range(0, self.n, 2 ** 27):  # (in pieces: the comparison's temporary stays at 128 MiB)
            touched += int((self.bits[c0:c0 + 2 ** 27] != SENTINEL).sum())
        assert touched == 0, f"{what}: {touched} elements of the arena outside the operand were written"


class Budget:
    """with Budget() as b: a = b.arena(...): the arenas of one test, at most CAP_BYTES together, dropped on exit"""

    def __enter__(self):
        self.arenas, self.bytes = [], 0
        return self

    def arena(self, *a, **kw):
        ar = Arena(*a, **kw)
        self.arenas.append(ar)
        self.bytes += ar.nbytes
        assert self.bytes <= CAP_BYTES, f"a test holds {self.bytes / 2 ** 30:.1f} GiB of arenas"
        return ar

    def __exit__(self, *exc):
        for ar in self.arenas:
            ar.buf = ar.bits = ar.view = None
        self.arenas = []
        torch.cuda.empty_cache()
        return False


def ints(shape, bound, seed):
    """integers in [-bound, bound] as doubles: sums of a few thousand products of them are exact in any order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g, dtype=torch.int64).double()


def refused(lib, rc, *names):
    """the call was refused as an invalid argument and the message names one of the leading dimensions"""
    msg = lib.pls_last_error().decode()
    assert rc == 1, f"status {rc} ({msg}), expected PLS_ERR_INVALID_ARGUMENT"
    assert "leading dimension" in msg and any(n in msg for n in names), msg
    return msg


def gemm_route(L, lib, l_ptr, ldl, r_ptr, ldr, ldc, i, j, k):
    """(route name or None when refused, direct_store)"""
    direct = ctypes.c_int32(-1)
    rc = lib.pls_gemm_tn_route(l_ptr, ldl, r_ptr, ldr, ldc, i, j, k, ctypes.byref(direct))
    return (L.GEMM_ROUTE_NAMES[rc] if rc >= 0 else None), direct.value
