"""The 50-digit truth of libplship's normal stream (csrc/philox.h) and the loader of tests/golden/philox_truth.npz (written by
tests/golden/make_philox_truth.py).  TEST INFRASTRUCTURE ONLY.

Element (row i, global column jg) of step ``step`` under ``seed``:
    (x0, x1, x2, x3) = Philox4x32-10({lo32(i with bit 2 cleared), lo32(jg), lo32(step), hi32(step)}, {lo32(seed), hi32(seed)})
    u1 = ((x0:x1 >> 11) + 1/2) 2^-53,  u2 = ((x2:x3 >> 11) + 1/2) 2^-53        (exact rationals)
    z  = sqrt(-2 ln u1) cos(2 pi u2)  on the rows with bit 2 clear,  ... sin(2 pi u2) on the rows with bit 2 set.
The integer words come from oracle/philox_ref.philox4x32_10 (exact; tests/test_oracle_goldens.py pins them with the Random123
known-answer vectors), the transform from mpmath at 50 digits.  A value is stored as its nearest double ``hi`` plus the
remainder ``lo`` (truth = hi + lo to ~2^-106 relative), so that an error can be counted in units of 2^-53 |truth| without a
rounding of the yardstick itself.

2 pi u2 = (pi / 4) (o + t): o = the top 3 bits of x2:x3 (the octant), t = ((the next 50 bits) + 1/2) 2^-50 the position in it."""
import os

import numpy as np

from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "philox_truth.npz")
DPS = 50

# the bulk: rows 0..15 of BULK_COLS columns from j_offset on, for each (seed, step, j_offset); the second has non-zero high
# words in seed and step, the fourth starts three columns before the column counter wraps (the stream is defined on lo32(jg))
BULK_ROWS, BULK_COLS = 16, 480
BULK_TRIPLES = [(1, 0, 0), (2**63 + 11, 2**33 + 3, 123456), (0xDEADBEEFCAFE, 5, 1000), (77, 2**32, 2**32 - 3)]

# the extremes: regimes of the host search (make_philox_truth.py), as stored in ext_regime
REGIMES = ["small u1", "u1 -> 1", *[f"octant {o} low edge" for o in range(8)], *[f"octant {o} high edge" for o in range(8)], "small |z|"]
R_SMALL_U1, R_U1_ONE, R_OCT_LOW, R_OCT_HIGH, R_SMALL_Z = 0, 1, 2, 10, 18
SEARCH_SEED, SEARCH_STEP = 0x1234_0000CAFE, 7  # the counters the search runs over: rows 0..3 (+4), columns below 2^26


def words(ibase, jg, step, seed):
    """the four Philox words of the pairs (ibase, jg) (arrays or numbers; ibase has bit 2 clear), as uint64 arrays"""
    ibase, jg = np.broadcast_arrays(np.asarray(ibase, dtype=np.uint64), np.asarray(jg, dtype=np.uint64))
    assert not (ibase & np.uint64(4)).any()
    step, seed = int(step), int(seed)
    return philox_ref.philox4x32_10(ibase, jg, np.full(ibase.shape, step & 0xFFFFFFFF, dtype=np.uint64),
                                    np.full(ibase.shape, (step >> 32) & 0xFFFFFFFF, dtype=np.uint64), seed & 0xFFFFFFFF,
                                    (seed >> 32) & 0xFFFFFFFF)


def uniforms53(x0, x1, x2, x3):
    """(a, b): the 53-bit integers of u1 = (a + 1/2) 2^-53 and u2 = (b + 1/2) 2^-53"""
    s32, s11 = np.uint64(32), np.uint64(11)
    return ((x0 << s32) | x1) >> s11, ((x2 << s32) | x3) >> s11


def octant_position(b):
    """(o, p): octant and the 50-bit integer of the position t = (p + 1/2) 2^-50 in it"""
    b = np.asarray(b, dtype=np.uint64)
    return (b >> np.uint64(50)).astype(np.int64), b & np.uint64((1 << 50) - 1)


def pair_truth(a, b):
    """((hi, lo) of the cos row, (hi, lo) of the sin row) for the 53-bit integers a, b of one pair"""
    import mpmath as mp

    with mp.workdps(DPS):
        half, scale = mp.mpf(1) / 2, mp.mpf(2) ** -53
        u1, u2 = (mp.mpf(int(a)) + half) * scale, (mp.mpf(int(b)) + half) * scale
        rad = mp.sqrt(-2 * mp.log(u1))
        ang = 2 * mp.pi * u2
        out = []
        for z in (rad * mp.cos(ang), rad * mp.sin(ang)):
            hi = float(z)  # (mpmath rounds to nearest)
            out.append((hi, float(z - mp.mpf(hi))))
        return tuple(out)


def element_truth(i, jg, step, seed):
    """(hi, lo) of one element from its counters"""
    x = words(int(i) & ~4, int(jg) & 0xFFFFFFFF, step, seed)
    a, b = uniforms53(*x)
    return pair_truth(a, b)[1 if int(i) & 4 else 0]


def units(got, hi, lo):
    """|got - truth| in units of 2^-53 |truth| (got - hi is exact for anything within a factor two of hi)"""
    got, hi, lo = (np.asarray(v, dtype=np.float64) for v in (got, hi, lo))
    return np.abs((got - hi) - lo) / (2.0 ** -53 * np.abs(hi))


def load():
    return dict(np.load(FIXTURE))
