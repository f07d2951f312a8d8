"""Host: the committed 50-digit truth of the normal stream (tests/golden/philox_truth.npz, tests/philox_truth.py) holds the
regimes the GPU tests need -- conditions on the file, not measurements --, re-evaluates from its counters, and shows why
oracle/philox_ref.normal_matrix (the numpy restatement) is not the yardstick of the transform."""
import numpy as np
import pytest

import philox_truth as T
from oracle import philox_ref


@pytest.fixture(scope="module")
def fx():
    return T.load()


def _ext_uniforms(fx):
    w = fx["ext_words"].astype(np.uint64)
    return T.uniforms53(w[:, 0], w[:, 1], w[:, 2], w[:, 3])


def test_fixture_shapes_and_counters(fx):
    nb = len(T.BULK_TRIPLES)
    assert fx["bulk_triples"].tolist() == [list(t) for t in T.BULK_TRIPLES]
    assert fx["bulk_hi"].shape == fx["bulk_lo"].shape == (nb, T.BULK_ROWS, T.BULK_COLS)
    assert any(seed >> 32 and step >> 32 for seed, step, _ in T.BULK_TRIPLES), "no bulk block with high words in seed and step"
    assert int(fx["search_pairs_log2"]) >= 27
    n = len(fx["ext_row"])
    for k in ("ext_col", "ext_step", "ext_seed", "ext_regime", "ext_hi", "ext_lo"):
        assert fx[k].shape == (n,)
    assert (fx["ext_col"] >= 0).all() and (fx["ext_col"] < 2**31).all(), "an extreme's column does not fit one 8 x 1 fill"
    assert (fx["ext_row"] >= 0).all() and (fx["ext_row"] < 8).all()
    for a in (fx["bulk_hi"], fx["ext_hi"]):
        assert np.isfinite(a).all() and (a != 0).all()
    for hi, lo in ((fx["bulk_hi"], fx["bulk_lo"]), (fx["ext_hi"], fx["ext_lo"])):
        assert (np.abs(lo) <= 2.0**-53 * np.abs(hi)).all(), "hi is not the nearest double"
    # the stored words are the stream's: every one recomputed from the counters (vectorised, exact)
    ibases = np.array([i for i in range(T.BULK_ROWS) if not i & 4], dtype=np.uint64)
    for t, (seed, step, joff) in enumerate(T.BULK_TRIPLES):
        jg = (np.arange(T.BULK_COLS, dtype=np.uint64) + np.uint64(joff)) & np.uint64(0xFFFFFFFF)
        want = np.stack(T.words(ibases[:, None], jg[None, :], step, seed), axis=-1)
        assert np.array_equal(fx["bulk_words"][t].astype(np.uint64), want), f"bulk block {t}: words"
    want = np.stack(T.words(fx["ext_row"] & ~4, fx["ext_col"], T.SEARCH_STEP, T.SEARCH_SEED), axis=-1)
    assert np.array_equal(fx["ext_words"].astype(np.uint64), want), "extremes: words"
    assert (fx["ext_step"] == T.SEARCH_STEP).all() and (fx["ext_seed"] == T.SEARCH_SEED).all()


def test_fixture_holds_every_regime(fx):
    a, b = _ext_uniforms(fx)
    o, p = T.octant_position(b)
    reg, row, col = fx["ext_regime"], fx["ext_row"], fx["ext_col"]
    assert set(o.tolist()) == set(range(8)), "an octant does not occur among the extremes"
    bo, _ = T.octant_position(T.uniforms53(*(fx["bulk_words"][..., k].astype(np.uint64) for k in range(4)))[1])
    assert set(bo.ravel().tolist()) == set(range(8)), "an octant does not occur in the bulk"
    # both rows (i and i + 4) of every pair kept, one after the other
    assert len(row) % 2 == 0
    assert ((row[0::2] & 4) == 0).all() and (row[1::2] == row[0::2] + 4).all() and (col[0::2] == col[1::2]).all()
    assert (reg[0::2] == reg[1::2]).all()
    # the sizes of the regimes
    count = lambda r: int((reg == r).sum()) // 2  # noqa: E731
    assert count(T.R_SMALL_U1) == 16 and count(T.R_U1_ONE) == 16 and count(T.R_SMALL_Z) == 16
    for oc in range(8):
        assert count(T.R_OCT_LOW + oc) == 4 and count(T.R_OCT_HIGH + oc) == 4
        assert (o[reg == T.R_OCT_LOW + oc] == oc).all() and (o[reg == T.R_OCT_HIGH + oc] == oc).all()
    # how far they reach: u1 = (a + 1/2) 2^-53 < 2^-24, 1 - u1 < 2^-24; t = (p + 1/2) 2^-50 < 2^-24 and 1 - t < 2^-24 in an even and
    # in an odd octant (the device reflects t in the odd ones)
    assert (a[reg == T.R_SMALL_U1] < 2**29).any(), "no u1 below 2^-24"
    assert ((2**53 - 1 - a[reg == T.R_U1_ONE].astype(np.int64)) < 2**29).any(), "no 1 - u1 below 2^-24"
    for parity in (0, 1):
        low = (reg >= T.R_OCT_LOW) & (reg < T.R_OCT_HIGH) & (o % 2 == parity)
        high = (reg >= T.R_OCT_HIGH) & (reg < T.R_SMALL_Z) & (o % 2 == parity)
        assert (p[low] < 2**26).any(), f"no t below 2^-24 in an octant of parity {parity}"
        assert ((2**50 - 1 - p[high].astype(np.int64)) < 2**26).any(), f"no 1 - t below 2^-24 in an octant of parity {parity}"
    small = np.abs(fx["ext_hi"][reg == T.R_SMALL_Z]).reshape(-1, 2).min(axis=1)
    assert (small < 2.0**-20).all(), "the small |z| entries are not small"


def test_entries_reproduce_from_their_counters(fx):
    rng = np.random.default_rng(5)
    nb = len(T.BULK_TRIPLES)
    for _ in range(150):
        t, i, c = int(rng.integers(nb)), int(rng.integers(T.BULK_ROWS)), int(rng.integers(T.BULK_COLS))
        seed, step, joff = T.BULK_TRIPLES[t]
        hi, lo = T.element_truth(i, joff + c, step, seed)
        assert hi == fx["bulk_hi"][t, i, c] and lo == fx["bulk_lo"][t, i, c], (t, i, c)
    for k in rng.choice(len(fx["ext_row"]), 50, replace=False).tolist():
        hi, lo = T.element_truth(fx["ext_row"][k], fx["ext_col"][k], int(fx["ext_step"][k]), int(fx["ext_seed"][k]))
        assert hi == fx["ext_hi"][k] and lo == fx["ext_lo"][k], k


def test_numpy_restatement_is_within_its_own_tolerance_and_no_truth(fx, record_property):
    """oracle/philox_ref.normal_matrix evaluates sin / cos(2 pi u2) of an angle rounded near 2 pi, with an absolute error: next to
    the zeros of sin and cos it is thousands of units of 2^-53 |z| off.  It stays inside the rtol 1e-12 / atol 1e-13 that
    test_philox_stream_matches_numpy_restatement grants it, which is all it is asked for; the transform is held to the truth."""
    worst, worst_abs = 0.0, 0.0
    for t, (seed, step, joff) in enumerate(T.BULK_TRIPLES):
        got = philox_ref.normal_matrix(T.BULK_ROWS, T.BULK_COLS, seed, step, joff)  # (the column wraps inside Philox: lo32)
        hi, lo = fx["bulk_hi"][t], fx["bulk_lo"][t]
        assert (np.abs(got - hi) <= 1e-13 + 1e-12 * np.abs(hi)).all(), f"bulk block {t}: the restatement left its own tolerance"
        worst = max(worst, float(T.units(got, hi, lo).max()))
        worst_abs = max(worst_abs, float(np.abs((got - hi) - lo).max()))
    for k in range(len(fx["ext_row"])):
        got = philox_ref.normal_matrix(8, 1, T.SEARCH_SEED, T.SEARCH_STEP, int(fx["ext_col"][k]))[fx["ext_row"][k], 0]
        hi, lo = fx["ext_hi"][k], fx["ext_lo"][k]
        assert abs(got - hi) <= 1e-13 + 1e-12 * abs(hi), f"extreme {k}: the restatement left its own tolerance"
        worst = max(worst, float(T.units(got, hi, lo)))
        worst_abs = max(worst_abs, abs((got - hi) - lo))
    record_property("restatement_worst_units", worst)
    record_property("restatement_worst_abs", worst_abs)
    print(f"numpy restatement against the truth: worst {worst:.3g} units of 2^-53 |z|, worst absolute {worst_abs:.3g}")
