"""CPU: tests/workspace_guards.py does not pass vacuously -- one flipped byte in either guard of a CPU-tensor Guarded is
reported at its offset relative to the region; a region that ends inside a word; outputs that start as the sentinel."""
import pytest
import torch

from workspace_guards import MIN_GUARD, SENTINEL, SENTINEL_BITS, Guarded, GuardedMatrix, guard_bytes, same_bits


def test_guard_sizes():
    assert [guard_bytes(n) for n in (0, 1000, 4 << 20, (4 << 20) + 8, 64 << 20, 1 << 30)] == \
        [4 << 20, 4 << 20, 4 << 20, (4 << 20) + 8, 64 << 20, 64 << 20]


@pytest.mark.parametrize("nbytes", [0, 8, 28, 1000 * 8, MIN_GUARD + 24])
@pytest.mark.parametrize("fill", [float("nan"), 1e300, 0.0, SENTINEL])
def test_a_flipped_guard_byte_is_reported_at_its_offset(nbytes, fill):
    g = Guarded(nbytes, fill, device="cpu")
    assert g.ptr % 256 == 0 and g.nbytes == nbytes and g.guard == guard_bytes(nbytes)
    assert g.start >= g.guard and g._bytes.numel() - g.end >= g.guard
    g.assert_intact("untouched")
    if nbytes % 8 == 0 and nbytes:
        if fill != fill:  # a plain NaN is not the sentinel; SENTINEL fills the region with the guards' own pattern
            assert g.f64().isnan().all() and bool((g.bits() == SENTINEL_BITS).all()) == (fill is SENTINEL)
        else:
            assert (g.f64() == fill).all()
    g.bytes().fill_(0x5A)  # the region itself is the library's to write: every byte of it
    g.assert_intact("region written")
    for off in (nbytes, nbytes + 1, nbytes + 7, nbytes + 8, nbytes + g.guard - 1, -1, -8, -9, -g.guard):
        at = g.start + off
        old = int(g._bytes[at])
        g._bytes[at] = old ^ 0x10
        assert g.first_damage() == off, (off, g.first_damage())
        with pytest.raises(AssertionError, match=f"offset {off} relative"):
            g.assert_intact("flipped")
        g._bytes[at] = old
        g.assert_intact("restored")
    # the first damaged byte: the front guard comes first
    g._bytes[g.start - 3] ^= 1
    g._bytes[g.end + 5] ^= 1
    assert g.first_damage() == -3


def test_outputs_counters_and_matrices():
    e = Guarded(8 * 10, SENTINEL, device="cpu")
    with pytest.raises(AssertionError, match="10 of 10 entries never written"):
        e.assert_written("nothing")
    e.f64()[:9] = 1.0
    with pytest.raises(AssertionError, match="first 9"):
        e.assert_written("a forgotten tail")
    e.assert_written("the head alone", count=9)
    e.f64()[9] = float("nan")  # (an ordinary NaN is a value, not the sentinel)
    e.assert_written("all")
    c = Guarded(4 * 7, 0.0, device="cpu")
    c.assert_zero("fresh counters")
    c.view(torch.int32)[6] = 1
    with pytest.raises(AssertionError, match="byte 24"):
        c.assert_zero("a counter left set")
    c.assert_intact("the last counter is inside the region")
    m = GuardedMatrix(4, 5, 8, device="cpu")
    assert m.nbytes == (3 * 8 + 5) * 8 and m.matrix().shape == (4, 5) and m.padding().shape == (3, 3)
    m.matrix().fill_(3.0)
    m.assert_written("every entry")
    m.assert_intact("every entry")
    assert (m.padding() == SENTINEL_BITS).all()
    m.f64()[8 + 6] = 0.0  # row 1, padding column 1
    with pytest.raises(AssertionError, match=r"padding behind column 5 was written, first \(row, pad column\) \[1, 1\]"):
        m.assert_written("padding")
    m.f64()[8 + 6] = SENTINEL
    m.matrix()[3, 4] = SENTINEL
    with pytest.raises(AssertionError, match=r"first \(row, column\) \[3, 4\]"):
        m.assert_written("the last entry")
    a, b = torch.tensor([float("nan"), 1.0], dtype=torch.float64), torch.tensor([SENTINEL, 1.0], dtype=torch.float64)
    assert same_bits(a, a.clone()) and not same_bits(a, b) and not torch.equal(a, a.clone())
