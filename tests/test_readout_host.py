"""Host: the restated summation orders of the read-out reductions (tests/readout_truth.py) stay inside their derived bounds
against exact integer sums, and trainers.mean_from_chunk_sums is pls_block_means' order on the host, bit for bit."""
import math

import numpy as np
import pytest

import readout_truth as T
from projected_langevin_sampling_amd import trainers

SIZES = [1, 15, 16, 17, 255, 256, 257, 513, 4097, 70001]


def test_exact_integers_reproduce_the_doubles():
    x = np.array([0.0, -0.0, 1.0, -3.5, 5e-324, -1e-310, 2.0 ** -1022, 1e300, -1e-300, 0.1])
    vals, e0 = T.ints_of(x)
    assert [float(v * T.scale(e0)) for v in vals] == x.tolist()
    ex = T.ExactVector([0.5, 0.25, -1.0, 3.0])
    assert ex.e0 == -2 - 52 and ex.sum() * T.scale(ex.e0) == T.Fraction(11, 4) and ex.abs_sum(1, 3) * T.scale(ex.e0) == T.Fraction(5, 4)
    assert ex.sum(2, 2) == 0
    num, mass, e0 = T.exact_power_sum([1.5, -0.5, 2.0], 2, 0.5)
    assert num == mass and num * T.scale(e0) == T.Fraction(17, 4)
    num, mass, e0 = T.exact_power_sum([1.5, -0.5, 2.0], 1, 0.5)
    assert (num * T.scale(e0), mass * T.scale(e0)) == (T.Fraction(3, 2), T.Fraction(7, 2))
    # the comparison itself, against the same quotient in fractions: fl(0.1 + 0.2) and the exact sum of the two doubles
    exact = T.Fraction(0.1) + T.Fraction(0.2)
    want = float(abs(T.Fraction(0.1 + 0.2) - exact) / (3 * T.Fraction(1, 2 ** 53) * exact))
    vals, e0 = T.ints_of([0.1, 0.2])
    assert 0.0 < want < 1.0 and T.error_in_bound(0.1 + 0.2, sum(vals), sum(vals), e0, 3) == pytest.approx(want, rel=1e-12)
    assert T.error_in_bound(0.1 + 0.2, 7 * sum(vals), 7 * sum(vals), e0, 3, div=7) == pytest.approx(want, rel=1e-12)
    assert T.error_in_bound(5e-324, 3, 3, -1000, 1) == pytest.approx((3 - 2.0 ** -74) / 3 * 2.0 ** 53)  # (a result below the unit)
    assert T.error_in_bound(1.0, 3, 0, 0, 5) == math.inf and T.error_in_bound(3.0, 3, 0, 0, 5) == 0.0


def test_the_orders_on_inputs_where_every_order_is_exact():
    """integers: each restatement is the plain sum, whatever its order; one lane, one chunk, one block off its place shows"""
    rng = np.random.default_rng(3)
    e = rng.integers(-1000, 1000, size=1000).astype(np.float64)
    assert T.chunk_sums(e).tolist() == [e[i:i + 256].sum() for i in range(0, 1000, 256)]
    assert T.sums16(e).tolist() == [e[i:i + 16].sum() for i in range(0, 1000, 16)]
    assert T.block_means(e * 1000, 96).tolist() == [e[i:i + 96].sum() * 1000 / len(e[i:i + 96]) for i in range(0, 1000, 96)]
    assert T.block_means(e).tolist() == [e.sum() / 1000]
    x = e.reshape(2, 500)
    assert T.row_power_sums(x, 1).tolist() == x.sum(1).tolist()
    assert T.row_power_sums(x, 2, np.array([3.0, -7.0])).tolist() == ((x - np.array([[3.0], [-7.0]])) ** 2).sum(1).tolist()
    assert T.row_power_sums(np.zeros((3, 0)), 2).tolist() == [0.0, 0.0, 0.0]


def test_the_butterfly_pairs_lanes_as_documented():
    """a wave whose sum depends on the pairing: 1 and two halves of its last bit, which vanish unless they meet each other
    before they meet the 1"""
    v = np.zeros(256)
    v[0], v[1], v[2] = 1.0, 2.0 ** -53, 2.0 ** -53
    # offsets 32 ... 4 add zeros; offset 2 pairs lanes 0, 2 and 1, 3; offset 1 then adds the two pairs
    assert T.chunk256_sum(v) == (1.0 + 2.0 ** -53) + (2.0 ** -53 + 0.0) == 1.0
    v[1], v[2], v[3] = 0.0, 2.0 ** -53, 2.0 ** -53
    assert T.chunk256_sum(v) == (1.0 + 2.0 ** -53) + (0.0 + 2.0 ** -53) == 1.0
    v[2], v[3], v[1] = 0.0, 2.0 ** -53, 2.0 ** -53  # lanes 1 and 3 meet at offset 2: their sum 2^-52 survives
    assert T.chunk256_sum(v) == 1.0 + 2.0 ** -52 > 1.0
    w = np.zeros(256)
    w[0], w[64], w[128], w[192] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53  # (w0 + w1) + (w2 + w3)
    assert T.chunk256_sum(w) == 1.0 + 2.0 ** -52
    # followed along lane 0 (the fast form) and with all 256 lanes carried, as the kernel does it
    x = T.log_spread((40, 256), seed=8)
    assert T.same_bits(T.chunk256_sum(x), T.chunk256_sum_all_lanes(x))
    for case in (v, w):
        assert T.same_bits(T.chunk256_sum(case), T.chunk256_sum_all_lanes(case))


@pytest.mark.parametrize("j", SIZES)
def test_restatements_stay_inside_the_bounds(j):
    e = T.log_spread(j, seed=j)
    ex = T.ExactVector(e)
    worst = {
        "chunk sums": max(T.chunk_sum_errors(T.chunk_sums(e), e, ex)),
        "sums16": max(T.sums16_errors(T.sums16(e), e, ex)),
        "block mean": max(T.block_mean_errors(T.block_means(e), e, ex=ex)),
    }
    for bc in (1, 16, 96, 255, 256, 257, 1000):
        worst[f"block means of {bc}"] = max(T.block_mean_errors(T.block_means(e, bc), e, bc, ex))
    x = T.log_spread((2, j), seed=j + 1)
    shift = 0.5 + 3.0 * np.random.default_rng(j + 2).standard_normal(2)
    worst["row sums"] = max(T.row_power_sum_errors(T.row_power_sums(x, 1, shift), x, 1, shift))
    mean = T.row_power_sums(x, 1) / j
    worst["row squares"] = max(T.row_power_sum_errors(T.row_power_sums(x, 2, mean), x, 2, mean))
    print(f"j = {j}: |error| / bound {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("j", [1, 255, 256, 257, 4096, 4097, 8192, 131072 + 257])
def test_mean_from_chunk_sums_is_the_block_mean_bit_for_bit(j):
    """both branches: at most 16 chunks (the loop, for a list and for an array) and more (np.cumsum)"""
    e = T.log_spread(j, seed=j)
    sums = T.chunk_sums(e)
    want = T.block_means(e)[0]
    assert (sums.size > 16) == (j > 4096)
    assert T.same_bits(trainers.mean_from_chunk_sums(sums, j), want)
    assert T.same_bits(trainers.mean_from_chunk_sums(sums.tolist(), j), want)
    # the 16-column sums of the one-launch step, through the same function: ascending adds from 0.0
    total = 0.0
    for v in T.sums16(e).tolist():
        total += v
    assert T.same_bits(trainers.mean_from_chunk_sums(T.sums16(e), j), total / j)


@pytest.mark.parametrize("chunks", [1, 16, 17])
def test_mean_from_chunk_sums_starts_from_plus_zero(chunks):
    """energies that are all -0.0: every chunk sum is -0.0, the kernel's total starts at +0.0 and stays there"""
    e = np.full(256 * chunks, -0.0)
    sums = T.chunk_sums(e)
    assert T.same_bits(sums, np.full(chunks, -0.0))
    want = T.block_means(e)[0]
    assert T.same_bits(want, 0.0)
    assert T.same_bits(trainers.mean_from_chunk_sums(sums, e.size), want)
    assert T.same_bits(trainers.mean_from_chunk_sums(sums.tolist(), e.size), want)
