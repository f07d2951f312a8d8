"""Host side of the read-out reductions: the documented summation orders of csrc/plship.hip restated in numpy, exact sums
to hold them (and the device) against, and the error bounds that follow from the orders alone.

Restatements (every add is one IEEE double add, in the order the kernel's comment states):

  chunk256_sum            xor butterfly with offsets 32, 16, 8, 4, 2, 1 inside each 64-lane group, then (w0 + w1) + (w2 + w3)
  pls_chunk_sums          the chunk sum of e[256 i, 256 (i + 1)), the last chunk padded with +0.0
  pls_block_means         per block of ``bc`` columns: chunks counted from the block's OWN first column, their sums added in
                          ascending order from 0.0, divided by the block's true length
  pls_sums16              sixteen ascending adds from 0.0 (missing columns add +0.0)
  row_power_sums_kernel   thread t adds (x - shift)^p of elements t, t + 256, ... in order from 0.0, then the 8-level tree
                          red[t] += red[t + w], w = 128 ... 1

Exact truths are integers: a double is m 2^e, so a vector is a list of Python ints at one common exponent (``ints_of``) and
its sums, sums of absolute values and sums of squared deviations are exact integer arithmetic, and so is the comparison
with a result (``error_in_bound``) up to its final quotient.

Bounds, u = 2^-53, each first-order count rounded up (gamma_n <= (n + 1) u for these n):

  chunk sum        9 u sum|e|                         (8 adds deep: 6 butterfly levels, 2 for the waves)
  block mean       (nchunk + 9) u sum|e| / len        (+ nchunk sequential adds, the division inside the slack)
  row power sum    (ceil(cols / 256) + 11) u sum|x - shift|^p
                                                      (the sequential adds, 8 tree levels, the subtraction, the square, slack)"""
import math
from fractions import Fraction

import numpy as np

_LANES = np.arange(256)


def cdiv(a, b):
    return -(-a // b)


def bits(x):
    """the bit patterns of doubles, as int64 (a scalar gives a 0-d array)"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def log_spread(shape, seed, sigma=6.0):
    """normals of both signs times exp(sigma N(0, 1)) -- magnitudes over some twenty decades -- with +0.0 and -0.0 mixed in"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * np.exp(sigma * rng.standard_normal(shape))
    flat = x.reshape(-1)
    if flat.size >= 8:  # (a handful of entries stay what they are)
        where = rng.integers(0, flat.size, size=flat.size // 16 + 1)
        flat[where[0::2]] = 0.0
        flat[where[1::2]] = -0.0
    return x


# ---- the documented orders --------------------------------------------------------------------------------------------------------
def chunk256_sum(v):
    """(..., 256) -> (...): the 256 lanes of one workgroup"""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[-1] == 256
    v = v.reshape(*v.shape[:-1], 4, 64)
    # v += shfl_xor(v, o) leaves lanes i and i ^ o with the SAME value v_i + v_(i ^ o) (an IEEE add commutes), so after the level
    # the lanes below o carry everything lane 0 will ever read: the butterfly, followed along lane 0 of each wave
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return (v[..., 0, 0] + v[..., 1, 0]) + (v[..., 2, 0] + v[..., 3, 0])


def chunk256_sum_all_lanes(v):
    """the same sum with every lane carried through the six levels, as the kernel does it (slow; the tests hold
    chunk256_sum to it)"""
    v = np.array(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ o]
    assert (v.reshape(*v.shape[:-1], 4, 64) == v.reshape(*v.shape[:-1], 4, 64)[..., :1]).all()  # (one value per wave)
    return (v[..., 0] + v[..., 64]) + (v[..., 128] + v[..., 192])


def chunk_sums(e):
    e = np.asarray(e, dtype=np.float64)
    n = cdiv(e.size, 256)
    pad = np.zeros(n * 256)
    pad[:e.size] = e
    return chunk256_sum(pad.reshape(n, 256))


def block_means(e, bc=None, batch=1 << 21):
    e = np.asarray(e, dtype=np.float64)
    j = e.size
    if j == 0:
        return np.zeros(0)
    bc = j if bc is None else int(bc)
    nb, nck = cdiv(j, bc), cdiv(min(bc, j), 256)
    t = np.arange(nck * 256)
    out = np.empty(nb)
    step = max(1, batch // (nck * 256))
    for b0 in range(0, nb, step):
        b = np.arange(b0, min(nb, b0 + step))
        c0 = b * bc
        ln = np.minimum(c0 + bc, j) - c0
        idx = c0[:, None] + t[None, :]
        v = np.where(t[None, :] < ln[:, None], e[np.minimum(idx, j - 1)], 0.0)
        sums = chunk256_sum(v.reshape(b.size, nck, 256))
        total = np.zeros(b.size)
        for k in range(nck):  # (a short last block's missing chunks add +0.0 to a total that is never -0.0: no change)
            total = total + sums[:, k]
        out[b] = total / ln
    return out


def sums16(e):
    e = np.asarray(e, dtype=np.float64)
    n = cdiv(e.size, 16)
    pad = np.zeros(n * 16)
    pad[:e.size] = e
    pad = pad.reshape(n, 16)
    s = np.zeros(n)
    for k in range(16):
        s = s + pad[:, k]
    return s


def row_power_sums(x, power, shift=None):
    """x: (rows, cols) without its padding.  power 2 squares with ONE rounding (no fused multiply-add)."""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = x.shape
    v = x - (0.0 if shift is None else np.asarray(shift, dtype=np.float64)[:, None])
    if power == 2:
        v = v * v
    trips = cdiv(cols, 256)
    pad = np.zeros((rows, trips * 256))  # (a missing element adds +0.0 to a sum that is never -0.0: no change)
    pad[:, :cols] = v
    pad = pad.reshape(rows, trips, 256)
    red = np.zeros((rows, 256))
    for k in range(trips):
        red = red + pad[:, k, :]
    w = 128
    while w > 0:
        red[:, :w] = red[:, :w] + red[:, w:2 * w]
        w >>= 1
    return red[:, 0].copy()


# ---- exact truths -------------------------------------------------------------------------------------------------------------------
def ints_of(x, also=()):
    """(list of Python ints k_i, exponent E) with x_i = k_i 2^E exactly; ``also``: more doubles that must fit the same E"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    assert np.isfinite(x).all()
    m, ex = np.frexp(np.concatenate([x, np.asarray(also, dtype=np.float64).reshape(-1)]))
    k = (m * 2.0 ** 53).astype(np.int64)  # (exact: 53 significant bits at most)
    ex = ex.astype(np.int64) - 53
    e0 = int(ex[k != 0].min()) if (k != 0).any() else 0
    vals = [int(a) << int(b - e0) if a else 0 for a, b in zip(k.tolist(), ex.tolist())]
    return vals, e0


def scale(e0):
    return Fraction(2) ** e0


def prefix(vals):
    out, s = [0], 0
    for v in vals:
        s += v
        out.append(s)
    return out


class ExactVector:
    """exact sums and sums of absolute values over any slice of a vector of doubles, as integers in units of 2^e0"""

    def __init__(self, e):
        vals, self.e0 = ints_of(e)
        self.n = len(vals)
        self._s, self._a = prefix(vals), prefix([abs(v) for v in vals])

    def sum(self, c0=0, c1=None):
        return self._s[self.n if c1 is None else c1] - self._s[c0]

    def abs_sum(self, c0=0, c1=None):
        return self._a[self.n if c1 is None else c1] - self._a[c0]


def exact_power_sum(row, power, shift=0.0):
    """(sum_k (row_k - shift)^power, sum_k |row_k - shift|^power, E): integers in units of 2^E"""
    vals, e0 = ints_of(row, also=[shift])
    sh = vals.pop()
    d = [v - sh for v in vals]
    if power == 1:
        return sum(d), sum(abs(v) for v in d), e0
    sq = sum(v * v for v in d)
    return sq, sq, 2 * e0


# ---- the bounds -----------------------------------------------------------------------------------------------------------------
def error_in_bound(got, num, mass, e0, k, div=1):
    """|got - truth| / bound for truth = num 2^e0 / div and bound = k u mass 2^e0 / div, in exact integer arithmetic up to the
    final quotient (0.0 where the error vanishes, inf where only the bound does): <= 1 passes"""
    got = float(got)
    assert math.isfinite(got), got
    m, ex = math.frexp(got)
    mg, eg = int(m * 2.0 ** 53), ex - 53
    low = min(e0, eg)
    err = abs((mg << (eg - low)) * div - (num << (e0 - low)))
    if err == 0:
        return 0.0
    bound = k * (mass << (e0 - low))  # (in units of u = 2^-53)
    return (err << 53) / bound if bound else math.inf


def chunk_sum_errors(got, e, ex=None):
    """per chunk |got - sum| / (9 u sum|e|)"""
    ex = ex or ExactVector(e)
    return [error_in_bound(g, ex.sum(256 * i, min(ex.n, 256 * i + 256)), ex.abs_sum(256 * i, min(ex.n, 256 * i + 256)), ex.e0, 9)
            for i, g in enumerate(np.asarray(got).tolist())]


def sums16_errors(got, e, ex=None):
    """per block of 16 |got - sum| / (17 u sum|e|): sixteen sequential adds, gamma_16 <= 17 u"""
    ex = ex or ExactVector(e)
    return [error_in_bound(g, ex.sum(16 * i, min(ex.n, 16 * i + 16)), ex.abs_sum(16 * i, min(ex.n, 16 * i + 16)), ex.e0, 17)
            for i, g in enumerate(np.asarray(got).tolist())]


def block_mean_errors(got, e, bc=None, ex=None):
    """per block |got - mean| / ((nchunk + 9) u sum|e| / len)"""
    ex = ex or ExactVector(e)
    bc = ex.n if bc is None else int(bc)
    out = []
    for b, g in enumerate(np.asarray(got, dtype=np.float64).reshape(-1).tolist()):
        c0, c1 = b * bc, min(ex.n, (b + 1) * bc)
        out.append(error_in_bound(g, ex.sum(c0, c1), ex.abs_sum(c0, c1), ex.e0, cdiv(c1 - c0, 256) + 9, div=c1 - c0))
    return out


def row_power_sum_errors(got, x, power, shift=None):
    """per row |got - sum (x - shift)^p| / ((ceil(cols / 256) + 11) u sum|x - shift|^p)"""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for r, g in enumerate(np.asarray(got).tolist()):
        num, mass, e0 = exact_power_sum(x[r], power, 0.0 if shift is None else float(shift[r]))
        out.append(error_in_bound(g, num, mass, e0, cdiv(x.shape[1], 256) + 11))
    return out
