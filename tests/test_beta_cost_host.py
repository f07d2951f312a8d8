"""CPU: the Beta cost without a GPU -- ids, descriptors, argument validation in the C ABI, the logit conversion, nativeness,
the predictive distribution, the checkpoint key, the metrics branches; and the truth of tests/beta_cost_truth.py: its grid,
the header's formula in (a, b) against the dedicated pair's form in mpmath, the derivative as the value's slope, the
recorded errors of the host restatement (tests/golden/beta_cost_reference_errors.json) against a fresh measurement, and the
regimes the selector problems of the route tests run through."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import beta_cost_truth as BT
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd import costs, link_functions, metrics
from step_fixtures import SelectorProblem

L = pkg._lib
Y = torch.tensor(BT.Y_ROWS, dtype=torch.float64)


def _cost(phi=3.0, link=None, y=None):
    return costs.BetaCost(Y if y is None else y, link or link_functions.SigmoidLinkFunction(), phi)


def test_ids_exports_and_abi():
    assert L.COST_BETA == 7 and L.COST_NEGATIVE_BINOMIAL == 5
    assert L.ABI_VERSION == 7 and L.load().pls_abi_version() == 7
    assert pkg.BetaCost is costs.BetaCost and "BetaCost" in costs.__all__ and "BetaCost" in pkg.__all__
    assert costs.BetaCost.cost_kind == L.COST_BETA


def test_descriptor_fields_in_both_modes():
    c = _cost(phi=12.5)
    assert c.observation_noise is None and c._params() == (12.5, 0.0, 0.0, 0.0) and c.precision == 12.5
    for fa, mode in ((False, L.DERIV_REFERENCE), (True, L.DERIV_AUTOGRAD)):
        d = c.desc(force_autograd=fa)
        assert (d.cost, d.link, d.deriv_mode) == (L.COST_BETA, L.LINK_SIGMOID, mode)
        assert list(d.p) == [12.5, 0.0, 0.0, 0.0] and d.jitter == 1e-10
    d = _cost(link=link_functions.ProbitLinkFunction()).desc()
    assert (d.cost, d.link) == (L.COST_BETA, L.LINK_PROBIT)


@pytest.mark.parametrize("phi", [0.0, -1.0, math.inf, math.nan])
def test_a_bad_precision_fails_before_any_hip_call(phi):
    lib = L.load()
    d = _cost(phi=phi).desc()
    assert lib.pls_cost_derivative(d, 8, 1, 8, 1, 1, 8, 1, None) == 1
    assert b"precision" in lib.pls_last_error()
    assert lib.pls_cost_value(d, 8, 1, 8, 1, 1, 8, None, 0, None) == 1
    assert b"precision" in lib.pls_last_error()


def test_the_new_id_passes_validation_and_six_is_still_refused():
    """cost id 7 is known: validation goes on to the pointers (all NULL here, so no HIP call follows); 6 and 99 are not"""
    lib = L.load()
    d = _cost().desc()
    assert lib.pls_cost_derivative(d, None, 1, None, 1, 1, None, 1, None) == 1
    assert b"NULL" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    for cost in (6, 99, -1):
        bad = L.CostDesc()
        bad.cost, bad.link, bad.p[0] = cost, L.LINK_SIGMOID, 1.0
        assert lib.pls_cost_derivative(bad, 8, 1, 8, 1, 1, 8, 1, None) == 1 and b"unknown cost" in lib.pls_last_error()
    assert lib.pls_debug_math(7, 8, 8, 1, None) == 1 and lib.pls_debug_math(-1, 8, 8, 1, None) == 1
    assert lib.pls_debug_math(6, None, None, 1, None) == 1 and b"bad arguments" in lib.pls_last_error()


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, math.nan])
def test_y_outside_the_open_interval_raises(bad):
    with pytest.raises(ValueError, match="strictly inside"):
        _cost(y=torch.tensor([0.3, bad, 0.6], dtype=torch.float64))
    with pytest.raises(ValueError, match="finite"):
        costs.BetaCost.from_logits(torch.tensor([0.0, math.inf]), link_functions.SigmoidLinkFunction(), 1.0)


def test_y_device_is_the_logit_and_y_train_is_untouched(monkeypatch):
    from projected_langevin_sampling_amd.costs import beta

    monkeypatch.setattr(beta, "_dev", lambda t: t)  # (no device here: the conversion itself)
    y = Y.clone()
    c = _cost(y=y)
    z = c.y_device()
    assert c.y_train is y and torch.equal(y, Y) and z.dtype == torch.float64 and c.y_device() is z
    for got, want in zip(z.tolist(), BT.Z_ROWS):
        assert abs(got - want) <= 2 * math.ulp(want), (got, want)
    c32 = _cost(y=torch.tensor([0.25, 0.75], dtype=torch.float32))
    assert c32.y_device().dtype == torch.float64 and c32.y_train.dtype == torch.float32
    assert torch.allclose(c32.y_device(), torch.tensor([-math.log(3.0), math.log(3.0)], dtype=torch.float64), rtol=1e-15)
    c.y_train = torch.tensor([0.5], dtype=torch.float64)  # a new y: a new logit
    assert c.y_device().tolist() == [0.0]
    # logits given: they are what the library gets, bit for bit, however near 0 or 1 the proportion lies
    zz = torch.tensor([-800.0, -3.0, 0.0, 40.0, 745.0], dtype=torch.float64)
    cz = costs.BetaCost.from_logits(zz, link_functions.SigmoidLinkFunction(), 2.0)
    assert torch.equal(cz.y_device(), zz) and bool(((cz.y_train > 0) & (cz.y_train < 1)).all())
    assert torch.allclose(cz.y_train[1:3], torch.sigmoid(zz[1:3]))


def test_is_native_unless_a_subclass_brings_its_own_torch_code():
    assert _cost().is_native() and _cost(link=link_functions.ProbitLinkFunction()).is_native()

    class Mine(costs.BetaCost):
        def calculate_cost(self, f):
            return f.sum(0)

    assert not Mine(Y, link_functions.SigmoidLinkFunction(), 1.0).is_native()

    class TorchLink(link_functions.PLSLinkFunction):
        def transform(self, y):
            return y.sigmoid()

    assert not _cost(link=TorchLink()).is_native()


def test_predict_returns_the_beta_with_the_samples_mean():
    g = torch.Generator().manual_seed(0)
    samples = torch.rand(5, 40, generator=g, dtype=torch.float64) * 0.9 + 0.05
    phi = 12.5
    dist = _cost(phi=phi).predict(samples)
    assert isinstance(dist, torch.distributions.Beta)
    mu = samples.mean(dim=1)
    assert torch.allclose(dist.mean, mu, rtol=1e-13) and torch.allclose(dist.variance, mu * (1 - mu) / (1 + phi), rtol=1e-12)
    assert torch.allclose(dist.concentration1 + dist.concentration0, torch.full((5,), phi, dtype=torch.float64), rtol=1e-15)


class _Stub:
    def __init__(self, cost):
        self.cost, self.basis = cost, None
    observation_noise = property(lambda s: s.cost.observation_noise, lambda s, v: setattr(s.cost, "observation_noise", v))


def test_checkpoint_round_trips_the_precision(tmp_path, monkeypatch):
    from projected_langevin_sampling_amd import checkpoint
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    path = str(tmp_path / "beta.pt")
    u = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    save_pls(_Stub(_cost(phi=1.0 / 3.0)), u, path, best_lr=1e-3, number_of_epochs=4)
    state = torch.load(path)
    assert state["precision"] == 1.0 / 3.0 and state["observation_noise"] is None and "dispersion" not in state
    save_pls(_Stub(costs.PoissonCost(torch.zeros(2), link_functions.SquareLinkFunction())), u, str(tmp_path / "p.pt"))
    assert "precision" not in torch.load(str(tmp_path / "p.pt"))
    monkeypatch.setattr(checkpoint, "_dev", lambda t: t)  # (no device here: load_pls would put the particles on it)
    other = _Stub(_cost(phi=9.0))
    _, got, lr, ep = load_pls(other, path)
    assert other.cost.precision == 1.0 / 3.0 and torch.equal(got.cpu(), u) and (lr, ep) == (1e-3, 4)


def test_metrics_take_beta_and_negative_binomial_predictions():
    y = torch.tensor([0.2, 0.7, 0.55], dtype=torch.float64)
    mu = torch.tensor([0.25, 0.6, 0.5], dtype=torch.float64)
    beta = torch.distributions.Beta(mu * 8.0, (1 - mu) * 8.0)
    assert metrics.calculate_mae(beta, y) == pytest.approx((mu - y).abs().mean().item(), rel=1e-12)
    assert metrics.calculate_mse(beta, y) == pytest.approx((mu - y).square().mean().item(), rel=1e-12)
    want = -sum(float(mp.log(mp.beta(a, b) ** -1 * mp.mpf(v) ** (a - 1) * (1 - mp.mpf(v)) ** (b - 1)))
                for a, b, v in zip((mu * 8).tolist(), ((1 - mu) * 8).tolist(), y.tolist())) / 3
    assert metrics.calculate_nll(beta, y) == pytest.approx(want, rel=1e-12)
    counts = torch.tensor([0.0, 3.0, 10.0], dtype=torch.float64)
    m, r = torch.tensor([1.5, 2.0, 7.0], dtype=torch.float64), torch.tensor(2.5, dtype=torch.float64)
    nb = torch.distributions.NegativeBinomial(total_count=r, probs=m / (r + m))
    assert metrics.calculate_mae(nb, counts) == pytest.approx((m - counts).abs().mean().item(), rel=1e-12)
    want = -sum(float(mp.log(mp.binomial(k + 2.5 - 1, k) * (mp.mpf(2.5) / (2.5 + mm)) ** 2.5 * (mm / (2.5 + mm)) ** k))
                for k, mm in zip(counts.tolist(), m.tolist())) / 3
    assert metrics.calculate_nll(nb, counts) == pytest.approx(want, rel=1e-12)


# ---- the truth ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,pset", BT.cells())
def test_grid_layout_and_regimes(pair, pset):
    z, f, regimes = BT.grid(pair, pset)
    n, j = f.shape
    assert n % 2 == 1 and j % 2 == 1 and z.shape == (n,) and len(regimes) == j
    assert list(z) == BT.Z_ROWS and BT.Y_ROWS == [0.5, 0.01, 0.999, 1.0 / 3.0, 1e-9, 1.0 - 2.0 ** -30, 0.2]
    for y, zz in zip(BT.Y_ROWS, z):
        assert abs(mp.mpf(zz) - (mp.log(mp.mpf(y)) - mp.log1p(-mp.mpf(y)))) <= mp.mpf(2) ** -53 * abs(mp.mpf(zz))
    col = lambda name: f[:, [b for b, r in enumerate(regimes) if r == name]]  # noqa: E731
    assert (np.abs(col("bulk")) <= 3).all()
    if pair == "beta/probit":
        assert set(regimes) == {"bulk", "wide"} and np.abs(col("wide")).max() == 8 and np.abs(col("wide")).min() > 3
        assert (np.abs(col("wide")) < 6.36).any() and (np.abs(col("wide")) > 6.37).any()  # both sides of the clip
        return
    assert set(regimes) == {"bulk", "centre", "root", "lo_tail", "hi_tail", "far", "zero"}
    assert (col("zero") == 0).any() and np.signbit(f[f == 0]).any() and (np.abs(col("zero")) < 2.3e-308).all() and (col("zero") != 0).any()
    assert np.abs(col("centre")).max() == 2.0 ** -8 and np.abs(col("centre")).min() == 2.0 ** -50
    assert col("hi_tail").min() == 30 and col("hi_tail").max() == 700 and col("lo_tail").max() == -30 and col("lo_tail").min() == -700
    assert {745.0, -745.0, 1e10, -1e10, 1e150, -1e150, 1e300, -1e300} == set(col("far").ravel())
    phi = mp.mpf(BT.PARAMS[pset])
    for a, zz in enumerate(z):
        fs = BT.root(pset, float(zz))
        if zz == 0.0:
            assert fs == 0.0
            continue
        # f* is the zero: the sign of the derivative changes across it, and the columns lie on both sides, 2^-8 .. 2^-50 away
        assert BT._slope_sign(phi, mp.mpf(zz), mp.mpf(fs) * (1 + mp.mpf(2) ** -45)) * BT._slope_sign(phi, mp.mpf(zz), mp.mpf(fs) * (1 - mp.mpf(2) ** -45)) < 0
        rel = np.abs(col("root")[a] / fs - 1)
        assert rel.min() < 2.0 ** -49 and rel.max() < 2.0 ** -7 and (col("root")[a] > fs).any() and (col("root")[a] < fs).any()


def test_the_parameter_sets_reach_what_they_are_for():
    assert BT.PARAMS == {"a": 0.3, "b": 400.0, "c": 3.0}
    assert abs(float(BT.PSI_ROOT) - 1.4616321449683623) < 1e-15


def test_the_header_formula_is_the_dedicated_form():
    """lgamma(a) + lgamma(b) - a z and phi (psi(a) - psi(b) - z) mu (1 - mu) against the form in e = exp(-|f|), in mpmath,
    where 1 - mu can be formed at the working precision (|f| <= 100); and the stated ends"""
    with mp.workdps(120):
        for pset, phi in BT.PARAMS.items():
            z, f, _ = BT.grid("beta/sigmoid", pset)
            for a in range(len(z)):
                for v in f[a][a % 2::2]:
                    if abs(v) > 100:  # (1 - mu keeps 40 digits of mu_s up to here; the ends are stated below)
                        continue
                    mu = 1 / (1 + mp.exp(-mp.mpf(v)))
                    v1, d1 = BT.beta_ab_form(mp.mpf(phi), mp.mpf(z[a]), phi * mu, phi * (1 - mu), mu * (1 - mu))
                    v2, d2, uv, ud = BT.beta_logit_form(phi, float(z[a]), float(v))
                    assert abs(v1 - v2) <= mp.mpf(10) ** -40 * uv, (pset, z[a], v)
                    assert abs(d1 - d2) <= mp.mpf(10) ** -40 * ud, (pset, z[a], v)
    # the tails: the issue's example, and a derivative of exactly +-1
    v = BT.beta_logit_form(0.3, 0.0, 745.0)[0]
    assert abs(v - (745 - mp.log(mp.mpf(0.3)) + mp.loggamma(mp.mpf(0.3)))) < mp.mpf(10) ** -40 and abs(float(v) - 747.3) < 0.05
    for s in (1, -1):
        v, d, _, _ = BT.beta_logit_form(3.0, 1.25, s * 1e300)
        assert d == s and abs(v / mp.mpf(1e300) - 1) < mp.mpf(10) ** -45
    for phi in BT.PARAMS.values():
        for ff in (40.0, -40.0, 60.0):
            assert abs(BT.beta_logit_form(phi, 0.0, ff)[1] - (1 if ff > 0 else -1)) < 2.0 ** -52 * max(1, phi)


def test_the_drift_is_bounded():
    """|cost'| <= 1 + phi (0.224 + |z| / 4).  The z-free part w (psi(a_b) - psi(a_s)) is at most w |f| + mu_b - mu_s / 2
    (log x - 1 / x <= psi(x) <= log x - 1 / (2 x), log(a_b / a_s) = |f|), and f mu (1 - mu) peaks at 0.2239 (f = 1.5434); the
    z part has w <= phi / 4.  (For phi of a few units and more the middle term is the larger one: the drift is bounded, by a
    constant that grows with phi, and tends to +-1 in the tails.)"""
    for phi in list(BT.PARAMS.values()) + [8.0, 1e6]:
        for k in range(0, 241):
            d = BT.beta_logit_form(phi, 0.0, k / 4.0)[1]
            assert 0 <= d <= 1 + 0.224 * phi, (phi, k, d)
        assert abs(BT.beta_logit_form(phi, 0.0, 60.0 + 2 * math.log(phi))[1] - 1) < 1e-15
    for pset, phi in BT.PARAMS.items():
        z, f, _ = BT.grid("beta/sigmoid", pset)
        for a in range(len(z)):
            for v in f[a]:
                assert abs(BT.beta_logit_form(phi, float(z[a]), float(v))[1]) <= 1 + phi * (0.224 + abs(z[a]) / 4)


def test_the_derivative_is_the_values_slope():
    with mp.workdps(130):
        for pair, pset in BT.cells():
            z, f, regimes = BT.grid(pair, pset)
            for a in range(len(z)):
                for b in range(a % 3, f.shape[1], 3):
                    zz, ff = float(z[a]), float(f[a, b])
                    if abs(ff) > 1e5:
                        continue
                    t, cu = BT.point_truth(pair, pset, "deriv", zz, ff)
                    if pair == "beta/probit" and t == 0 and abs(ff) > 6.3:
                        continue  # (clipped: the slope is 0 as autograd sees it, not the value's)
                    h = mp.mpf(2) ** -70 * abs(mp.mpf(ff)) if ff != 0 else mp.mpf(2) ** -1200
                    vp = BT.point_truth(pair, pset, "value", zz, mp.mpf(ff) + h)[0]
                    vm = BT.point_truth(pair, pset, "value", zz, mp.mpf(ff) - h)[0]
                    num = (vp - vm) / (2 * h)
                    tol = mp.mpf(2) ** -40 * cu / BT.U + (abs(vp) + 1) / h * mp.mpf(2) ** -400
                    assert abs(num - t) <= tol, (pair, pset, regimes[b], zz, ff, num, t)


def test_host_restatement_against_truth_matches_the_recorded_errors():
    """A fresh run of the restatement on the grid against the file: torch's vectorised functions differ by an ulp between CPU
    generations, so fresh and recorded must agree within a factor of two plus one unit (as tests/test_count_cost_host.py holds
    its restatement); no cell is a miss, and both derivative modes are the same numbers."""
    fresh, rec = BT.measure_reference(), BT.reference_errors()
    assert set(rec) == set(BT.PAIRS) | {"special"} and {(p, s) for p in BT.PAIRS for s in rec[p]} == set(BT.cells())
    for pair, pset in BT.cells():
        assert set(fresh[pair][pset]) == set(rec[pair][pset]) == set(BT.KINDS)
        assert rec[pair][pset]["deriv_reference"] == rec[pair][pset]["deriv_autograd"]
        for kind, cells in fresh[pair][pset].items():
            assert set(cells) == set(rec[pair][pset][kind]) == set(BT.grid(pair, pset)[2])
            for regime, v in cells.items():
                r = rec[pair][pset][kind][regime]
                assert r != "inf" and math.isfinite(v) and r < BT.T.ORACLE_MISS, (pair, pset, kind, regime, v, r)
                assert v <= 2 * r + 1 and r <= 2 * v + 1, (pair, pset, kind, regime, v, r)
    assert set(rec["special"]) == set(BT.SPECIALS)
    for name, cells in fresh["special"].items():
        assert set(cells) == set(rec["special"][name]) == set(BT.special_points(name)[1])
        for regime, v in cells.items():
            r = rec["special"][name][regime]
            assert math.isfinite(v) and r < BT.T.ORACLE_MISS and v <= 2 * r + 1 and r <= 2 * v + 1, (name, regime, v, r)
    assert all(BT.bound(v) <= 4e3 for p in BT.PAIRS for s in rec[p] for k in rec[p][s] for v in rec[p][s][k].values())


def test_special_points_cover_their_ranges():
    for name in BT.SPECIALS:
        x, regimes = BT.special_points(name)
        assert len(x) == len(regimes) and 2000 <= len(x) <= 5000 and (x > 0).all()
        assert x.max() > 1e290 and (x.min() < 1e-290 if name != "digamma" else x.min() >= 1.0)
        for c in (1.0, float(BT.PSI_ROOT), 2.0):
            near = np.abs(x - c)
            assert ((near < 2.0 ** -40) & (near > 0)).any() and ((near > 2.0 ** -12) & (near < 2.0 ** -7)).any()


def test_host_cost_drives_the_oracle_unchanged():
    """the restatement is duck-typed like the oracle's costs: oracle.pls_oracle.PLS and train_pls take it"""
    from oracle import pls_oracle as O

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(40, 1, generator=g) * 2 - 1
        zi = x[:6].clone()
        y = torch.sigmoid(1.5 * x[:, 0] + 0.3 * torch.randn(40, generator=g))
        ob = O.OrthonormalBasis(O.RBFARDKernel(torch.tensor([0.4]), 1.0), zi, x, 1e-2)
        oc = BT.BetaHostCost(torch.logit(y), BT.SigmoidLink(), 5.0)
        u = 0.1 * torch.randn(ob.approximation_dimension, 5, generator=g)
        out, energies = O.train_pls(O.PLS(ob, oc), u.clone(), 5, 1e-4, 1e9, noises=[torch.zeros_like(u)] * 5)
        assert len(energies) == 5 and energies[-1] < energies[0] and torch.isfinite(out).all()
    finally:
        torch.set_default_dtype(prev)


def test_the_selector_problems_run_through_the_regimes():
    for pair in BT.PAIRS:
        ex = SelectorProblem(pair, 17, 333, 600, "head", seed=1)
        f = ex.f()
        assert (f.abs() < 3).any() and (f.abs() > 6.4).any() and (f > 0).any() and (f < 0).any()
        assert set(ex.y.tolist()) == set(BT.Z_ROWS)
    f = SelectorProblem("beta/sigmoid", 17, 333, 600, "head", seed=1).f()
    assert (f.abs() > 1e9).any() and (f.abs() < 2.0 ** -20).any() and ((f.abs() > 700) & (f.abs() < 1e4)).any()
