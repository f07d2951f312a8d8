"""Guarded device buffers for the tests of the memory the library is LENT (tests/test_gpu_workspace_bounds.py): workspaces
sized by a pls_*_workspace_bytes query, the side buffers whose size include/plship.h states, and outputs.

``Guarded(nbytes, fill)`` is ONE allocation of the test's own,

    [front guard | region of exactly nbytes, 256-byte aligned | back guard]

whose guards hold one fixed 64-bit pattern (SENTINEL_BITS: a quiet NaN with a payload no computation produces) and are
compared as int64.  The library is given ``.ptr`` and ``.nbytes`` -- the queried byte count, never the tensor's size -- so a
store one row past the end lands in the back guard instead of the caching allocator's slack, and ``assert_intact`` reports
it as a byte offset relative to the region (negative: the front guard).

Guard size: each guard is min(max(nbytes, 4 MiB), 64 MiB) (at least: the front guard also takes the alignment padding).
This is a condition, not a measurement: a detected overrun must land in memory the test owns.  The widest row of tiles any
kernel stores at the shapes of the test file is 128 rows of a G chunk or of a Winograd plane of J = 2048 columns, 128 x 2048
x 8 = 2 MiB (every other cell: 128 x 1100 x 8 < 1.1 MiB), below the 4 MiB minimum; a whole region mis-based by its own size
stays inside a guard of nbytes; the Winograd cell's buffers (hundreds of MiB) take the 64 MiB cap, 32 rows of tiles.

The region starts as ``fill``: a NaN, 1e300 or 0.0 for memory whose contents the library must not depend on (a NaN shows a
stale read that propagates, the large finite value one that fmax or a comparison would swallow), 0.0 for the counters the
header wants zero on entry, or SENTINEL (the guards' own pattern) for outputs: after the call ``assert_written`` demands
that no sentinel remains among the entries the header says are written -- a forgotten tail block fails it."""
import torch

SENTINEL_BITS = 0x7FF8C0DEFACE5EED
SENTINEL = torch.tensor([SENTINEL_BITS], dtype=torch.int64).view(torch.float64).item()  # (as a double: a quiet NaN)
_SENTINEL_BYTES = torch.tensor([SENTINEL_BITS], dtype=torch.int64).view(torch.uint8)
MIN_GUARD, MAX_GUARD, ALIGN = 4 << 20, 64 << 20, 256

FILLS = [float("nan"), 1e300, 0.0]  # the three contents a lent region is run with


def guard_bytes(nbytes):
    return min(max(int(nbytes), MIN_GUARD), MAX_GUARD)


def _is_sentinel(fill):
    return isinstance(fill, float) and fill != fill and \
        torch.tensor([fill], dtype=torch.float64).view(torch.int64).item() == SENTINEL_BITS


class Guarded:
    def __init__(self, nbytes, fill, device="cuda"):
        self.nbytes = nbytes = int(nbytes)
        assert nbytes >= 0
        g = self.guard = guard_bytes(nbytes)
        words = (g + ALIGN + nbytes + g + 7) // 8 + 1
        self._words = torch.full((words,), SENTINEL_BITS, dtype=torch.int64, device=device)
        self._bytes = self._words.view(torch.uint8)
        base = self._words.data_ptr()
        assert base % 8 == 0
        self.start = (base + g + ALIGN - 1) // ALIGN * ALIGN - base  # byte offset of the region: front guard >= g bytes
        self.end = self.start + nbytes
        self.ptr = base + self.start
        assert self.ptr % ALIGN == 0 and self.start >= g and self._bytes.numel() - self.end >= g
        self.fill = fill
        if not _is_sentinel(fill):
            whole = nbytes // 8
            if whole:
                self._words[self.start // 8: self.start // 8 + whole].view(torch.float64).fill_(fill)
            if nbytes % 8:  # (a region that ends inside a word: 32-bit counters, byte maps)
                self._bytes[self.start + whole * 8: self.end].fill_(0 if fill == 0.0 else 0xFF)

    # ---- views of the region ----------------------------------------------------------------------------------------------
    def bytes(self):
        return self._bytes[self.start: self.end]

    def view(self, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % size == 0, (self.nbytes, dtype)
        return self.bytes().view(dtype)

    def f64(self):
        return self.view(torch.float64)

    def bits(self):
        return self.view(torch.int64)

    # ---- the checks -------------------------------------------------------------------------------------------------------
    def first_damage(self):
        """byte offset, relative to the region, of the first guard byte that no longer holds the pattern; None: intact"""
        w0, w1 = self.start // 8, (self.end + 7) // 8
        front = (self._words[:w0] != SENTINEL_BITS).nonzero()
        if front.numel():
            return self._byte_in_word(int(front[0])) - self.start
        if self.end % 8:  # the word the region ends in: its bytes behind the region
            pat = _SENTINEL_BYTES.to(self._bytes.device)[self.end % 8:]
            bad = (self._bytes[self.end: w1 * 8] != pat).nonzero()
            if bad.numel():
                return self.nbytes + int(bad[0])
        back = (self._words[w1:] != SENTINEL_BITS).nonzero()
        if back.numel():
            return self._byte_in_word(w1 + int(back[0])) - self.start
        return None

    def _byte_in_word(self, w):
        bad = (self._bytes[w * 8: w * 8 + 8] != _SENTINEL_BYTES.to(self._bytes.device)).nonzero()
        return w * 8 + int(bad[0])

    def assert_intact(self, what):
        off = self.first_damage()
        if off is None:
            return
        where = f"{-off} bytes in front of" if off < 0 else f"{off - self.nbytes} bytes behind the end of"
        raise AssertionError(f"{what}: guard damaged at offset {off} relative to the region of {self.nbytes} bytes ({where} it)")

    def assert_zero(self, what):
        """counters the header wants zero on entry and promises zero on return"""
        bad = self.bytes().nonzero()
        assert bad.numel() == 0, f"{what}: not zero after the call, first at byte {int(bad[0])} of {self.nbytes}"

    def assert_written(self, what, count=None):
        """an output that started as SENTINEL: none may remain among its first ``count`` doubles (default: all)"""
        b = self.bits() if count is None else self.bits()[:count]
        left = (b == SENTINEL_BITS).nonzero()
        assert left.numel() == 0, f"{what}: {left.numel()} of {b.numel()} entries never written, first {int(left[0])}"


class GuardedMatrix(Guarded):
    """A rows x cols output with leading dimension ld >= cols inside a Guarded of exactly ((rows - 1) ld + cols) doubles:
    the last row has no padding behind it.  The padding columns of the other rows hold the sentinel and must keep it."""

    def __init__(self, rows, cols, ld, fill=SENTINEL, device="cuda"):
        assert ld >= cols and rows >= 1
        self.rows, self.cols, self.ld = rows, cols, ld
        super().__init__(((rows - 1) * ld + cols) * 8, fill, device)

    def matrix(self, dtype=torch.float64):
        return self.view(dtype).as_strided((self.rows, self.cols), (self.ld, 1))

    def padding(self):
        return self.bits()[self.cols:].as_strided((self.rows - 1, self.ld - self.cols), (self.ld, 1))

    def assert_written(self, what, count=None):
        left = (self.matrix(torch.int64) == SENTINEL_BITS).nonzero()
        assert left.numel() == 0, f"{what}: {left.shape[0]} entries never written, first (row, column) {left[0].tolist()}"
        if self.rows > 1 and self.ld > self.cols:
            hit = (self.padding() != SENTINEL_BITS).nonzero()
            assert hit.numel() == 0, f"{what}: the padding behind column {self.cols} was written, first (row, pad column) {hit[0].tolist()}"


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
