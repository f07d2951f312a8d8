"""CPU: the per-element truth of tests/cost_truth.py -- its grid, its distance from the clip discontinuities, the oracle
measured against it, and the recorded measurement (tests/golden/cost_truth_oracle_errors.json) the GPU tests take their
bounds from."""
import math

import mpmath as mp
import numpy as np
import pytest

import cost_truth as T
from cost_families import family_cells, truth_module


@pytest.mark.parametrize("pair,pset", T.cells())
def test_grid_layout_and_regimes(pair, pset):
    """N and J off every multiple of 4 (so of 64), every row its own y with mixed labels, the regimes the pair needs"""
    y, f, regimes = T.grid(pair, pset)
    n, j = f.shape
    assert n % 2 == 1 and j % 2 == 1 and y.shape == (n,) and len(regimes) == j
    cost, link = pair.split("/")
    need = {"bernoulli": {"bulk", "lo_tail", "hi_tail", "clip_lo", "clip_hi", "clipped", "p_near_y", "zero"},
            "poisson": {"bulk", "pole", "root", "tail", "zero"}, "multimodal": {"bulk", "tie", "underflow", "absorbed", "zero"},
            "student_t": {"bulk", "e_small", "e_large", "zero"},
            "gaussian": {"bulk", "root", "tail", "zero"} if link == "square" else {"bulk", "e_small", "e_large", "zero"}}[cost]
    assert need <= set(regimes)
    bulk = f[:, [b for b, r in enumerate(regimes) if r == "bulk"]]
    if link != "identity":
        assert (np.abs(bulk) < 3).all()
    assert (f[:, [b for b, r in enumerate(regimes) if r == "zero"]] == 0).any() and np.signbit(f[f == 0]).any()
    if cost == "bernoulli":
        assert {0.0, 1.0} <= set(y) and ((y > 0) & (y < 1)).any()
        assert any(set(y[i:i + 4]) >= {0.0, 1.0} for i in range(0, n - 3))  # four consecutive rows with mixed labels
        assert np.abs(f).max() >= 745
    if cost == "poisson":
        assert {0.0, 1.0, 1e6} <= set(y) and 0 < np.abs(f[f != 0]).min() < 1e-300 and (np.abs(f) == 1e-300).any()
    if pair in ("gaussian/identity", "student_t/identity"):
        assert np.abs(f).max() >= 1e150


@pytest.mark.parametrize("pair,pset", [c for c in T.cells() if c[0].startswith("bernoulli")])
def test_no_point_near_a_clip_discontinuity(pair, pset):
    """In mpmath: every point's unclipped link value is at least 2^-44 (relative) away from jitter and 1 - jitter, and at
    least 8 units of the resolution fp64 has there (2^-53 x the terms the value is formed from: probit's 1 + erf resolves
    its lower tail absolutely).  So no fp64 evaluation can misjudge the side, and no point is excluded."""
    rel, res = T.clip_distances(pair, pset)
    assert len(rel) > 40
    assert rel.min() >= T.CLIP_MARGIN, rel.min()
    assert res.min() >= 8.0, res.min()
    # and the grid does hold points on both sides of both bounds, as near as 2^-40 (2^-14 / 2^-28 for probit's lower bound)
    _, f, regimes = T.grid(pair, pset)
    link, jit = pair.split("/")[1], T.PARAMS[pset]["jitter"]
    for name, b in (("clip_lo", jit), ("clip_hi", 1.0 - jit)):
        raws = [T.link_truth(link, v, jit) for v in np.unique(f[:, [i for i, r in enumerate(regimes) if r == name]])]
        assert any(r[3] for r in raws) and any(not r[3] for r in raws), name
        nearest = min(float(abs(r[0] - mp.mpf(b)) / mp.mpf(b)) for r in raws)
        assert nearest < (2.0 ** -13 if (link == "probit" and name == "clip_lo") else 2.0 ** -39), (name, nearest)


def test_truth_identities():
    """the truth against itself: the derivative is the value's slope (central difference in mpmath) wherever the reference
    differentiates, and the closed form of Bernoulli/sigmoid equals it inside the clip but not outside"""
    with mp.workdps(130):  # (the difference quotient divides the values' own rounding by h)
        _check_slopes()
    t_in, _ = T.point_truth("bernoulli/sigmoid", "a", "deriv_reference", 1.0, 2.0)
    t_auto, _ = T.point_truth("bernoulli/sigmoid", "a", "deriv_autograd", 1.0, 2.0)
    assert abs(t_in - t_auto) < mp.mpf(10) ** -45
    t_out, _ = T.point_truth("bernoulli/sigmoid", "a", "deriv_reference", 1.0, -40.0)
    assert T.point_truth("bernoulli/sigmoid", "a", "deriv_autograd", 1.0, -40.0)[0] == 0 and abs(t_out + 1) < 1e-9


def _check_slopes():
    for pair, pset in T.cells():
        y, f, regimes = T.grid(pair, pset)
        for a in range(0, len(y), 3):
            for b in range(0, f.shape[1], 2):
                yy, ff = float(y[a]), float(f[a, b])
                if ff == 0.0 and pair.startswith("poisson"):
                    continue
                t, cu = T.point_truth(pair, pset, "deriv_autograd", yy, ff)
                h = mp.mpf(2) ** -70 * abs(mp.mpf(ff)) if ff != 0 else mp.mpf(2) ** -1200
                vp = _value_at(pair, pset, yy, mp.mpf(ff) + h)
                vm = _value_at(pair, pset, yy, mp.mpf(ff) - h)
                num = (vp - vm) / (2 * h)
                # (h^2 of truncation, 2^-166 of the values' own rounding; cu / 2^-53 holds the sizes of the terms that cancel)
                tol = mp.mpf(2) ** -40 * cu / T.U + (abs(vp) + 1) / h * mp.mpf(2) ** -400
                assert abs(num - t) <= tol, (pair, pset, regimes[b], yy, ff, num, t)


def _value_at(pair, pset, y, f):
    cost, link = pair.split("/")
    prm = T.PARAMS[pset]
    _, p, slope, _, _ = T.link_truth(link, f, prm["jitter"])
    return T._from_p(cost, link, "value", prm, mp.mpf(y), f, p, slope)[0]


def test_specials_at_the_poisson_pole():
    for link in ("square", "identity"):
        pair = f"poisson/{link}"
        assert T.point_truth(pair, "a", "value", 3.0, 0.0)[0] == math.inf and math.isnan(T.point_truth(pair, "a", "value", 0.0, -0.0)[0])
        assert math.isnan(T.point_truth(pair, "a", "deriv_autograd", 3.0, 0.0)[0])
    assert T.point_truth("poisson/square", "a", "deriv_reference", 3.0, 0.0)[0] == -math.inf
    assert T.point_truth("poisson/square", "a", "deriv_reference", 3.0, -0.0)[0] == math.inf
    assert math.isnan(T.point_truth("poisson/square", "a", "deriv_reference", 0.0, 0.0)[0])
    assert math.isnan(T.point_truth("poisson/identity", "a", "deriv_reference", 3.0, 0.0)[0])


def test_error_measure():
    tr = {"hi": np.array([[1.0, math.inf, math.nan, 0.0, 1.0]]), "lo": np.array([[2.0 ** -54, 0, 0, 0, 0]]),
          "unit": np.array([[2.0 ** -52, math.nan, math.nan, 2.0 ** -1074, 2.0 ** -52]])}
    e = T.errors(np.array([[1.0 + 2.0 ** -52, math.inf, math.nan, 0.0, math.nan]]), tr)[0]
    assert e[0] == 0.75 and e[1] == 0 and e[2] == 0 and e[3] == 0 and e[4] == math.inf
    e = T.errors(np.array([[1.0, -math.inf, 1.0, 5e-324, math.inf]]), tr)[0]
    assert e[0] == 0.25 and e[1] == math.inf and e[2] == math.inf and e[3] == 1 and e[4] == math.inf


def test_oracle_against_truth_matches_the_recorded_errors():
    """A fresh run of the oracle on the grid against the file.  torch's vectorised exp / log / erf differ by an ulp between
    CPU generations, so a cell may move: fresh and recorded must agree within a factor of two plus one unit, and the same
    cells must be the ones the oracle misses outright."""
    fresh, rec = T.measure_oracle(), T.reference_errors()
    assert {(p, s) for p in rec for s in rec[p]} == set(T.cells())
    for pair, pset in T.cells():
        assert set(fresh[pair][pset]) == set(rec[pair][pset]) == {k for k in T.KINDS if T.applies(pair, k)}
        for kind, cells in fresh[pair][pset].items():
            assert set(cells) == set(rec[pair][pset][kind]) == set(T.grid(pair, pset)[2])
            for regime, v in cells.items():
                r = rec[pair][pset][kind][regime]
                what = (pair, pset, kind, regime, v, r)
                if r == "inf" or math.isinf(v):
                    assert r == "inf" and math.isinf(v), what
                else:
                    assert v <= 2 * r + 1 and r <= 2 * v + 1, what
    # the cells the oracle misses are its two known artefacts and nothing else
    missed = {(p, k, r) for p in rec for s in rec[p] for k in rec[p][s] for r, v in rec[p][s][k].items() if v == "inf" or v > T.ORACLE_MISS}
    assert missed == {("bernoulli/sigmoid", "deriv_autograd", "overflow"), ("multimodal/identity", "deriv_autograd", "absorbed")}


def test_bound_rule():
    assert T.bound(0.3) == 4 and T.bound(35.0) == 140 and T.bound("inf") == 4 and T.bound(5.6e15) == 4
    rec = T.reference_errors()
    assert all(T.bound(v) <= 4e4 for p in rec for s in rec[p] for k in rec[p][s] for v in rec[p][s][k].values())


# ---- the selector problems of tests/step_fixtures.py: their exactness, proved on the host ---------------------------------------
def _host_g(ex):
    """G on the problem's F by the host cost of the pair's truth module (the oracle's, or the family's restatement)"""
    import torch

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return truth_module(ex.pair).host_cost(ex.pair, ex.pset, ex.y).calculate_cost_derivative(ex.f())
    finally:
        torch.set_default_dtype(prev)


def _selector_problem_shows_g(pair, pset, mk, n, j, placement):
    import torch

    from step_fixtures import BLOCK_ETAS, EXACT_ETA, SelectorProblem, assert_selector

    ex = SelectorProblem(pair, mk, n, j, placement, seed=mk + n, pset=pset)
    assert len(ex.probe_k) == min(mk - 1, n) or placement == "spread"
    g = _host_g(ex)
    etas = torch.tensor(BLOCK_ETAS)[torch.arange(j) % 4]
    for eta in (EXACT_ETA, etas):
        e = torch.as_tensor(eta, dtype=torch.float64).expand(j)[None, :]
        for step in (-e * (ex.a @ g) - e * ex.u / ex.lam[:, None],
                     -e * (ex.a.flip(1) @ g.flip(0)) - e * ex.u / ex.lam[:, None]):
            assert_selector(ex, step, g, eta=eta, what=f"{pair} host")
            assert_selector(ex, ex.u + step, g, eta=eta, new_state=True, what=f"{pair} host, new state")
    # a fault of one ulp in one probe's G, or a probe reading its neighbour's row, does not pass
    bad = -EXACT_ETA * (ex.a @ g)
    k, nk = int(ex.probe_k[0]), int(ex.probe_n[0])
    col = int((g[nk] != 0).nonzero()[0])
    bad[k, col] = np.nextafter(float(bad[k, col]), math.inf)
    with pytest.raises(AssertionError):
        assert_selector(ex, bad, g, what="mutant")


@pytest.mark.parametrize("pair", T.PAIRS)
@pytest.mark.parametrize("mk,n,j,placement", [(10, 100, 64, "head"), (17, 333, 37, "spread"), (120, 1530, 200, "tail"),
                                              (129, 1200, 110, "half"), (12, 40, 5, "spread"), (200, 90, 33, "head")])
def test_selector_problem_shows_g_bit_for_bit(pair, mk, n, j, placement):
    """The fixture's own checks (F exact in either summation order, one power-of-two entry per probe direction), and the
    construction's claim on the host: with G the oracle's derivative on F, the step written out in fp64 torch, in two
    summation orders, shows -eta 2^p G[n_k, :] on every probe row without a rounding, and the carrier row within its
    bound."""
    _selector_problem_shows_g(pair, "a", mk, n, j, placement)


@pytest.mark.parametrize("pair,pset", family_cells())
@pytest.mark.parametrize("mk,n,j,placement", [(10, 100, 64, "head"), (17, 333, 37, "spread"), (120, 1530, 200, "tail"), (12, 40, 5, "spread")])
def test_selector_problem_shows_g_bit_for_bit_in_every_family(pair, pset, mk, n, j, placement):
    """the same proof for the pairs of every family's truth module (tests/cost_families.py), with G each module's host cost's"""
    _selector_problem_shows_g(pair, pset, mk, n, j, placement)


def test_selector_values_run_through_the_regimes():
    from step_fixtures import SelectorProblem

    for pair in T.PAIRS:
        ex = SelectorProblem(pair, 17, 333, 600, "head", seed=1)
        f = ex.f().numpy()
        cost, link = pair.split("/")
        assert (np.abs(f) < 3).any() and (np.abs(f) > 20).any() and (f > 0).any() and (f < 0).any()
        if link in ("sigmoid", "probit"):
            raw = np.array([float(T.link_truth(link, v, 1e-10)[0]) for v in f[0, ::7]])
            assert (raw < 1e-10).any() and (raw > 1 - 1e-10).any() and ((raw > 1e-10) & (raw < 1e-3)).any()
            assert set(ex.y.tolist()) >= {0.0, 1.0} and ((ex.y > 0) & (ex.y < 1)).any()
        if cost == "poisson":
            assert (np.abs(f) < 1e-9).any() and {0.0, 1.0, 1e6} <= set(ex.y.tolist())


def _selector_ipb_problem_shows_g(pair, pset, m, n, j, placement):
    import torch

    from step_fixtures import EXACT_ETA, SelectorIpbProblem, assert_selector

    ex = SelectorIpbProblem(pair, m, n, j, placement, seed=m + n, pset=pset)
    lc = torch.linalg.cholesky(ex.kzz)
    assert torch.equal(lc, torch.diag(ex.d)) and torch.equal(lc @ lc.T, ex.kzz)
    v = torch.cholesky_solve(ex.u, lc)
    assert torch.equal(ex.kzx.T @ v, ex.f()) and (v[torch.arange(m) != ex.k0] == 0).all() and torch.equal(v[ex.k0], ex.v)
    g = _host_g(ex)
    step = -EXACT_ETA * (ex.kzx @ g + m * v)
    assert_selector(ex, step, g, what="host")
    assert_selector(ex, ex.u + step, g, new_state=True, what="host, new state")
    ex.whitened()
    assert_selector(ex, step / ex.d[:, None], g, what="host, whitened")
    assert_selector(ex, ex.s + step / ex.d[:, None], g, new_state=True, what="host, whitened, new state")


@pytest.mark.parametrize("pair", ["poisson/square", "bernoulli/probit", "multimodal/identity"])
@pytest.mark.parametrize("m,n,j,placement", [(17, 333, 37, "tail"), (64, 1000, 100, "head"), (200, 300, 33, "half")])
def test_selector_ipb_problem_shows_g_bit_for_bit(pair, m, n, j, placement):
    """the inducing-point form: k(Z,Z) = diag(4^e) factorises, inverts and solves exactly, V holds the carrier values on one
    row, and the step -- written out in fp64 torch, plain and in whitened coordinates -- shows G on its probe rows"""
    _selector_ipb_problem_shows_g(pair, "a", m, n, j, placement)


@pytest.mark.parametrize("pair,pset", family_cells())
def test_selector_ipb_problem_shows_g_bit_for_bit_in_every_family(pair, pset):
    _selector_ipb_problem_shows_g(pair, pset, 17, 333, 37, "tail")
