"""CPU: the Gamma cost without a GPU -- the descriptor, argument validation in the C ABI (every refusal with its own message,
before any HIP call), the Python-side refusals, the logarithm handed to the library, nativeness, estimate_concentration, the
predictive distribution's moments, the two metrics, the checkpoint key, the ids; and the truth of tests/gamma_cost_truth.py:
its grid, the library's cost against the full negative log-likelihood in mpmath, the derivative as the value's slope, the
host restatement against the truth on every cell and on the non-finite z the grid cannot hold, its recorded errors
(tests/golden/gamma_cost_reference_errors.json) against a fresh measurement, and the selector problems of both parameter sets."""
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest
import torch

from cost_families import truth_module
import gamma_cost_truth as CT
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd import costs, link_functions, metrics
from step_fixtures import SelectorProblem

L = pkg._lib
INF = math.inf
PAIR = "gamma/exp"


class _HostP:
    """what tests/gamma_cost_truth.py needs of the GPU tests' package fixture to build the library's cost object"""
    costs, links = costs, link_functions


@pytest.fixture
def host_dev(monkeypatch):
    """no device here: the conversion of y itself"""
    from projected_langevin_sampling_amd.costs import gamma

    monkeypatch.setattr(gamma, "_dev", lambda t: t)


def _cost(k=2.5, link=None, y=None):
    y = torch.tensor([0.5, 1.0, 7.25], dtype=torch.float64) if y is None else y
    return costs.GammaCost(y, link or link_functions.ExponentialLinkFunction(), concentration=k)


def _desc(k, link=None):
    d = L.CostDesc()
    d.cost, d.link, d.deriv_mode = L.COST_GAMMA, L.LINK_EXP if link is None else link, L.DERIV_REFERENCE
    d.p[0] = k
    d.jitter = 1e-10
    return d


def test_ids_exports_and_abi():
    assert L.COST_GAMMA == 11
    assert L.ABI_VERSION == 7 and L.load().pls_abi_version() == 7
    assert pkg.GammaCost is costs.GammaCost and "GammaCost" in costs.__all__ and "GammaCost" in pkg.__all__
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "plship.h")).read()
    assert re.search(r"PLS_COST_GAMMA\s*=\s*11\b", header) and "10 is not a kind" in header


def test_descriptor_fields():
    c = _cost(0.75)
    assert c.observation_noise is None and c.concentration == 0.75 and c._params() == (0.75, 0.0, 0.0, 0.0)
    assert not hasattr(c, "shape")  # (the parameter is torch's ``concentration``: a cost never grows a float .shape)
    for fa, mode in ((False, L.DERIV_REFERENCE), (True, L.DERIV_AUTOGRAD)):
        d = c.desc(force_autograd=fa)
        assert (d.cost, d.link, d.deriv_mode) == (L.COST_GAMMA, L.LINK_EXP, mode) and list(d.p) == [0.75, 0.0, 0.0, 0.0]


REFUSALS = [
    (0.0, None, b"shape (concentration) > 0"),
    (-1.0, None, b"shape (concentration) > 0"),
    (INF, None, b"finite shape"),
    (math.nan, None, b"finite shape"),
    (2.5, L.LINK_IDENTITY, b"exponential link"),
    (2.5, L.LINK_SQUARE, b"exponential link"),
    (2.5, L.LINK_SIGMOID, b"exponential link"),
    (2.5, L.LINK_PROBIT, b"exponential link"),
]


@pytest.mark.parametrize("k,link,word", REFUSALS)
def test_a_bad_descriptor_fails_before_any_hip_call(k, link, word):
    """(the pointers are not device memory: a kernel launched on them would fault, a refusal returns first)"""
    lib = L.load()
    d = _desc(k, link)
    assert lib.pls_cost_derivative(d, 8, 1, 8, 1, 1, 8, 1, None) == 1
    assert word in lib.pls_last_error() and b"gamma" in lib.pls_last_error()
    assert lib.pls_cost_value(d, 8, 1, 8, 1, 1, 8, None, 0, None) == 1
    assert word in lib.pls_last_error() and b"gamma" in lib.pls_last_error()


def test_the_new_id_passes_validation():
    """cost id 11 is known and 10 is not: validation goes on to the pointers (all NULL here, so no HIP call follows)"""
    lib = L.load()
    for k in (2.5, 0.05, 1e-300, 1e300):
        assert lib.pls_cost_derivative(_desc(k), None, 1, None, 1, 1, None, 1, None) == 1
        assert b"NULL" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error() and b"gamma" not in lib.pls_last_error()
    bad = _desc(2.5)
    for kind in (6, 8, 10, 12):
        bad.cost = kind
        assert lib.pls_cost_derivative(bad, 8, 1, 8, 1, 1, 8, 1, None) == 1 and b"unknown cost" in lib.pls_last_error()


def test_python_side_refusals():
    exp = link_functions.ExponentialLinkFunction()
    for bad in (0.0, -1.0, INF, math.nan):
        with pytest.raises(ValueError, match="finite and > 0"):
            costs.GammaCost(torch.tensor([1.0, bad, 2.0], dtype=torch.float64), exp, concentration=1.0)
    for bad in (0.0, -2.0, INF, math.nan):
        with pytest.raises(ValueError, match="concentration"):
            _cost(bad)
    for link in (link_functions.IdentityLinkFunction(), link_functions.SquareLinkFunction(), link_functions.SigmoidLinkFunction(),
                 link_functions.ProbitLinkFunction()):
        with pytest.raises(ValueError, match="ExponentialLinkFunction"):
            _cost(link=link)
    with pytest.raises(ValueError, match="finite"):
        costs.GammaCost.from_logs(torch.tensor([0.0, INF]), exp, 1.0)
    c = _cost()
    with pytest.raises(ValueError, match="concentration"):
        c.concentration = 0.0
    assert c.concentration == 2.5
    assert costs.GammaCost(torch.tensor([1, 2, 3]), exp, concentration=1).concentration == 1.0  # integer dtypes


def test_y_device_is_the_logarithm_and_from_logs_round_trips(host_dev):
    y = torch.tensor([0.5, 1.0, 7.25, 1e-300, 1e300], dtype=torch.float64)
    keep = y.clone()
    c = _cost(y=y)
    z = c.y_device()
    assert c.y_train is y and torch.equal(y, keep) and z.dtype == torch.float64 and c.y_device() is z
    for got, yy in zip(z.tolist(), y.tolist()):
        want = float(mp.log(mp.mpf(yy)))
        assert abs(got - want) <= math.ulp(want), (got, want)
    c32 = _cost(y=torch.tensor([0.25, 4.0], dtype=torch.float32))
    assert c32.y_device().dtype == torch.float64 and c32.y_train.dtype == torch.float32
    assert torch.allclose(c32.y_device(), torch.tensor([-math.log(4.0), math.log(4.0)], dtype=torch.float64), rtol=1e-15)
    c.y_train = torch.tensor([1.0], dtype=torch.float64)  # a new y: a new logarithm
    assert c.y_device().tolist() == [0.0]
    # logarithms given: they are what the library gets, bit for bit, also beyond the fp64 range of y
    zz = torch.tensor([-800.0, -3.0, 0.0, 40.0, 745.0], dtype=torch.float64)
    cz = costs.GammaCost.from_logs(zz, link_functions.ExponentialLinkFunction(), 2.0)
    assert torch.equal(cz.y_device(), zz) and bool((torch.isfinite(cz.y_train) & (cz.y_train > 0)).all())
    assert torch.allclose(cz.y_train[1:4], torch.exp(zz[1:4])) and cz.concentration == 2.0
    back = costs.GammaCost.from_logs(_cost(y=y[:3]).y_device(), link_functions.ExponentialLinkFunction(), 2.5)
    assert torch.allclose(back.y_train, y[:3], rtol=4e-16) and torch.equal(back.y_device(), torch.log(y[:3]))


def test_is_native_unless_a_subclass_brings_its_own_torch_code():
    assert _cost().is_native()

    class Mine(costs.GammaCost):
        def calculate_cost(self, f):
            return f.sum(0)

    assert not Mine(torch.ones(2), link_functions.ExponentialLinkFunction(), concentration=1.0).is_native()


# ---- estimate_concentration ------------------------------------------------------------------------------------------------------
def _residual(k, s):
    k = mp.mpf(k)
    return abs(mp.log(k) - mp.digamma(k) - mp.mpf(s))


@pytest.mark.parametrize("s", [1e-6, 1e-3, 0.02, 0.3, 1.0, 4.0, 30.0, 300.0])
def test_the_concentration_solves_its_equation(s):
    k = costs.GammaCost._solve_concentration(s)
    assert k > 0 and math.isfinite(k) and _residual(k, s) <= 1e-12, (s, k, _residual(k, s))


def test_estimate_concentration_on_data():
    g = torch.Generator().manual_seed(3)
    mu = torch.exp(0.5 * torch.randn(4000, generator=g, dtype=torch.float64))
    ks = []
    for k_true in (0.3, 2.5, 40.0):
        y = torch._standard_gamma(torch.full((4000,), k_true, dtype=torch.float64), generator=g) / k_true * mu
        ratio = y / mu
        s = float((ratio - torch.log(ratio) - 1).mean())
        k = costs.GammaCost.estimate_concentration(y, mu)
        assert _residual(k, s) <= 1e-12 and abs(k / k_true - 1) < 0.1, (k_true, k)
        ks.append(k)
    assert ks[0] < ks[1] < ks[2]
    # one mean for all; float32 and integer inputs
    y = torch.tensor([1.0, 2.0, 4.0])
    s = float(np.mean([r - math.log(r) - 1 for r in (0.5, 1.0, 2.0)]))
    assert _residual(costs.GammaCost.estimate_concentration(y, torch.tensor(2.0)), s) <= 1e-12
    assert costs.GammaCost.estimate_concentration(torch.tensor([1, 2, 4]), 2.0) == costs.GammaCost.estimate_concentration(y, torch.tensor(2.0))


def test_the_concentration_is_monotone_in_s():
    """log k - psi(k) falls with k: a larger s (more spread) gives a smaller k"""
    ss = [10.0 ** e for e in np.linspace(-6, 2.5, 60)]
    ks = [costs.GammaCost._solve_concentration(s) for s in ss]
    assert all(a > b for a, b in zip(ks, ks[1:]))
    assert abs(ks[0] * 2 * ss[0] - 1) < 1e-3 and abs(ks[-1] * ss[-1] - 1) < 0.05  # k ~ 1 / (2 s) and ~ 1 / s at the two ends


def test_estimate_concentration_refuses_what_has_no_maximum():
    y = torch.tensor([0.5, 2.0, 3.0], dtype=torch.float64)
    with pytest.raises(ValueError, match="every y equals its mean"):
        costs.GammaCost.estimate_concentration(y, y.clone())
    with pytest.raises(ValueError, match="finite and > 0"):
        costs.GammaCost.estimate_concentration(torch.tensor([1.0, 0.0]), torch.tensor([1.0, 1.0]))
    with pytest.raises(ValueError, match="finite and > 0"):
        costs.GammaCost.estimate_concentration(y, torch.tensor([1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="as many means"):
        costs.GammaCost.estimate_concentration(y, torch.tensor([1.0, 1.0]))


# ---- prediction, metrics, checkpoint -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_predict_moments(pset):
    k = CT.PARAMS[pset]
    samples = torch.tensor([[0.5, 1.5, 4.0], [1e-3, 1e-3, 1e-3], [30.0, 10.0, 20.0]], dtype=torch.float64)  # (n, J) link values
    dist = _cost(k).predict(samples)
    mu = samples.mean(dim=1)
    assert isinstance(dist, torch.distributions.Gamma) and dist.mean.shape == (3,)
    assert torch.allclose(dist.mean, mu, rtol=1e-15) and torch.allclose(dist.variance, mu * mu / k, rtol=1e-15)
    assert torch.equal(dist.concentration, torch.full((3,), k, dtype=torch.float64)) and torch.allclose(dist.rate, k / mu, rtol=1e-15)
    yy = torch.tensor([0.7, 2e-3, 25.0], dtype=torch.float64)
    for a in range(3):
        want = -CT.full_nll(k, float(yy[a]), float(mu[a]))
        assert abs(mp.mpf(float(dist.log_prob(yy)[a])) - want) <= 1e-12 * (1 + abs(want))


def test_the_two_metrics_of_a_gamma_prediction():
    dist = torch.distributions.Gamma(concentration=torch.tensor([2.0, 0.5], dtype=torch.float64), rate=torch.tensor([4.0, 0.25], dtype=torch.float64))
    y = torch.tensor([1.0, 1.0])
    assert torch.equal(metrics._point(dist), torch.tensor([0.5, 2.0], dtype=torch.float64))  # the mean
    assert metrics.calculate_mae(dist, y) == (0.5 + 1.0) / 2
    assert metrics.calculate_mse(dist, y) == (0.25 + 1.0) / 2
    want = -(float(-CT.full_nll(2.0, 1.0, 0.5)) + float(-CT.full_nll(0.5, 1.0, 2.0))) / 2
    assert abs(metrics.calculate_nll(dist, y) - want) < 1e-14


def test_checkpoint_round_trips_the_concentration(tmp_path):
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    class Stub:
        def __init__(self, cost):
            self.cost, self.basis = cost, None
        observation_noise = property(lambda s: s.cost.observation_noise, lambda s, v: setattr(s.cost, "observation_noise", v))

    path = str(tmp_path / "gamma.pt")
    u = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    save_pls(Stub(_cost(1.0 / 3.0)), u, path, best_lr=1e-3, number_of_epochs=4)
    state = torch.load(path)
    assert state["concentration"] == 1.0 / 3.0 and state["observation_noise"] is None
    assert "dispersion" not in state and "precision" not in state and "cutpoints" not in state

    class Plain:
        basis = None
        cost = costs.PoissonCost(torch.zeros(2), link_functions.SquareLinkFunction())
        observation_noise = None

    save_pls(Plain(), torch.zeros(2, 2), str(tmp_path / "p.pt"))
    assert "concentration" not in torch.load(str(tmp_path / "p.pt"))
    if not torch.cuda.is_available():
        return  # (load_pls puts the particles on the device: tests/test_gpu_family_cost_train.py loads)
    other = Stub(_cost(9.0))
    _, got, lr, ep = load_pls(other, path)
    assert other.cost.concentration == 1.0 / 3.0 and torch.equal(got.cpu(), u) and (lr, ep) == (1e-3, 4)


# ---- the truth ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,pset", CT.cells())
def test_grid_layout_and_regimes(pair, pset):
    z, f, regimes = CT.grid(pair, pset)
    n, j = f.shape
    assert n % 2 == 1 and j % 2 == 1 and z.shape == (n,) and len(regimes) == j
    assert set(regimes) == {"bulk", "root", "round", "over", "under", "nonfinite"}
    assert np.isfinite(z).all() and (np.abs(z) <= 30).all() and set(z) == set(CT.Z_ROWS)
    col = lambda name: np.array([b for b, r in enumerate(regimes) if r == name])  # noqa: E731
    with mp.workdps(60):
        t = np.array([[float(mp.mpf(z[a]) - mp.mpf(f[a, b])) if np.isfinite(f[a, b]) else math.nan for b in range(j)] for a in range(n)])
    assert (np.abs(t[:, col("bulk")]) <= 30.001).all() and (t[:, col("bulk")] > 0).any() and (t[:, col("bulk")] < 0).any()
    root = t[:, col("root")]
    assert (root == 0).any() and (np.abs(root) <= 1e-6 * 31).all()
    for a in range(n):  # both signs, from 1e-6 |z| down to one ulp of z
        nz = root[a][root[a] != 0]
        assert (nz > 0).any() and (nz < 0).any() and np.abs(nz).min() <= 2 * math.ulp(z[a]) and np.abs(nz).max() >= 0.9e-6 * abs(z[a])
    tiny = np.abs(z[:, None] - f[:, col("root")])[z == 3 * 2.0 ** -1023]  # (exact in fp64: subnormal differences)
    assert tiny[tiny > 0].min() == 5e-324 and tiny.max() < 2.0 ** -1022
    rnd = t[:, col("round")]
    assert (np.abs(rnd) > 100).all() and rnd.max() > 700 and rnd.min() < -700
    # the subtraction rounds there: fl(z - f) is not the real z - f in most cells
    fl = z[:, None] - f[:, col("round")]
    assert (np.array([[mp.mpf(fl[a, b]) != mp.mpf(z[a]) - mp.mpf(f[a, cb]) for b, cb in enumerate(col("round"))] for a in range(n)])).mean() > 0.5
    over = np.sort(np.unique(np.round(t[:, col("over")], 2)))
    assert list(over) == [709.7, 709.78, 709.79, 710.0, 1e6]
    under = np.unique(np.round(t[:, col("under")], 0))
    assert set(under) >= {-36.0, -38.0, -745.0, -746.0, -1e9, -1e300}
    nf = f[:, col("nonfinite")]
    assert np.isnan(nf).any() and (nf == INF).any() and (nf == -INF).any() and not np.isfinite(nf).any()
    assert np.isfinite(np.delete(f, col("nonfinite"), axis=1)).all()


def test_the_cost_is_the_full_nll_without_its_constant():
    """-log Gamma(y; k, mean e^f) = k (e^t - t) + [z + lgamma(k) - k log k], t = z - f with z = log y, in mpmath"""
    with mp.workdps(80):
        for pset, k in CT.PARAMS.items():
            for y in (1e-5, 0.3, 1.0, 7.5, 2e6):
                z = mp.log(mp.mpf(y))
                const = z + mp.loggamma(k) - mp.mpf(k) * mp.log(mp.mpf(k))
                for f in [x / 4 for x in range(-80, 81)]:
                    cost = mp.mpf(k) * (mp.exp(z - f) - (z - f))
                    nll = CT.full_nll(k, y, mp.exp(mp.mpf(f)))
                    assert abs(nll - (cost + const)) <= mp.mpf(10) ** -60 * (abs(nll) + 1), (pset, y, f)
    # the header's statements about the minimum and the range
    v, d = CT.gamma_form(2.5, 0.0)
    assert v == 2.5 and d == 0
    assert all(CT.gamma_form(2.5, t)[0] > 2.5 and CT.gamma_form(2.5, t)[1] < 2.5 for t in (-100.0, -1.0, -1e-9, 1e-9, 1.0, 700.0))
    assert CT.gamma_form(0.05, 709.79) == (INF, -INF) and CT.gamma_form(0.05, 709.78)[0] < mp.mpf(2) ** 1024
    assert CT.gamma_form(2.5, -1e300) == (mp.mpf(2.5) * mp.mpf(1e300), 2.5)


def test_the_derivative_is_the_values_slope():
    with mp.workdps(130):
        for pair, pset in CT.cells():
            z, f, regimes = CT.grid(pair, pset)
            for a in range(len(z)):
                for b in range(f.shape[1]):
                    zz, ff = float(z[a]), float(f[a, b])
                    if not math.isfinite(ff) or abs(zz - ff) > 709:
                        continue
                    t, _ = CT.point_truth(pair, pset, "deriv_autograd", zz, ff)
                    assert t == CT.point_truth(pair, pset, "deriv_reference", zz, ff)[0] and t <= CT.PARAMS[pset]
                    k, tt = mp.mpf(CT.PARAMS[pset]), mp.mpf(zz) - mp.mpf(ff)
                    h = mp.mpf(2) ** -100
                    num = (k * (mp.exp(tt - h) - (tt - h)) - k * (mp.exp(tt + h) - (tt + h))) / (2 * h)  # (d/df = -d/dt)
                    assert abs(num - t) <= mp.mpf(2) ** -180 * (1 + k * mp.exp(tt) + abs(tt)), (pair, pset, regimes[b], zz, ff)


def test_host_restatement_against_truth_on_every_cell():
    """no cell of the restatement is further than a few units from the truth at the exact real z - f -- with the corrected t;
    the same formulas on the rounded t alone miss the round regime by hundreds of units -- and every special is the stated one"""
    fresh = CT.measure_reference()
    for pair, pset in CT.cells():
        for kind in CT.KINDS:
            for regime, v in fresh[pair][pset][kind].items():
                assert v <= 3.0, (pair, pset, kind, regime, v)
        z, f, regimes = CT.grid(pair, pset)
        k = CT.PARAMS[pset]
        hi = torch.as_tensor(z)[:, None] - torch.as_tensor(f)
        plain = {"value": k * (torch.exp(hi) - hi), "deriv_reference": -k * torch.expm1(hi)}
        for kind, got in plain.items():
            with np.errstate(invalid="ignore"):
                err = CT.by_regime(CT.errors(got.numpy(), CT.truth(pair, pset, kind)), regimes)
            assert err["round"] > 100 and err["root"] <= 3.0, (pair, pset, kind, err)


NONFINITE_Z = [(INF, 0.3), (INF, -1e300), (INF, -INF), (-INF, 0.3), (-INF, 1e300), (-INF, INF), (math.nan, 0.3), (math.nan, INF),
               (0.3, math.nan), (INF, INF), (-INF, -INF), (INF, math.nan)]


@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_the_edges_of_the_header_in_truth_and_restatement(pset):
    """the table of include/plship.h, also for the non-finite z the grid cannot hold: +inf / -inf where t is +inf, +inf / k
    where it is -inf, NaN for a NaN (and for z and f infinite with the same sign)"""
    k = CT.PARAMS[pset]
    want = {(INF, 0.3): (INF, -INF), (INF, -INF): (INF, -INF), (-INF, 0.3): (INF, k), (-INF, INF): (INF, k), (0.3, -INF): (INF, -INF),
            (0.3, INF): (INF, k), (0.3, 0.3 - 710.0): (INF, -INF), (0.3, 0.3 - 1e6): (INF, -INF), (0.3, 1e300): (2.5e300 if k == 2.5 else 5e298, k),
            (0.3, 0.3 + 746.0): (k * 746.0, k)}
    for (z, f), (v, d) in want.items():
        got = tuple(float(CT.point_truth(PAIR, pset, kind, z, f)[0]) for kind in ("value", "deriv_reference"))
        assert got == pytest.approx((v, d), rel=1e-15), (z, f, got)
    pts = NONFINITE_Z + list(want)
    z = np.array([p[0] for p in pts])
    f = np.array([[p[1]] for p in pts])
    for kind in CT.KINDS:
        got = np.array([CT.host_eval(PAIR, pset, kind, z[a:a + 1], f[a:a + 1])[0, 0] for a in range(len(pts))])
        for a, (zz, ff) in enumerate(pts):
            t = CT.point_truth(PAIR, pset, kind, zz, ff)[0]
            if isinstance(t, float):
                assert (math.isnan(t) and math.isnan(got[a])) or got[a] == t, (kind, zz, ff, got[a], t)
            else:
                assert abs(mp.mpf(got[a]) - t) <= 4 * CT.U * abs(t), (kind, zz, ff, got[a], t)
    assert math.isnan(CT.point_truth(PAIR, pset, "value", INF, INF)[0]) and math.isnan(CT.point_truth(PAIR, pset, "value", 0.3, math.nan)[0])


def test_the_recorded_errors_are_current():
    """A fresh run of the restatement on the grid against the file: torch's vectorised exp / expm1 differ by an ulp between CPU
    generations, so fresh and recorded must agree within a factor of two plus one unit (as tests/test_ordinal_cost_host.py
    holds its restatement); no cell is a miss, and both derivative modes are the same numbers."""
    fresh, rec = CT.measure_reference(), CT.reference_errors()
    assert {(p, s) for p in rec for s in rec[p]} == set(CT.cells())
    for pair, pset in CT.cells():
        assert set(fresh[pair][pset]) == set(rec[pair][pset]) == set(CT.KINDS)
        assert rec[pair][pset]["deriv_reference"] == rec[pair][pset]["deriv_autograd"]
        for kind, cells in fresh[pair][pset].items():
            assert set(cells) == set(rec[pair][pset][kind]) == set(CT.grid(pair, pset)[2])
            for regime, v in cells.items():
                r = rec[pair][pset][kind][regime]
                assert r != "inf" and math.isfinite(v) and r <= 3.0, (pair, pset, kind, regime, v, r)
                assert v <= 2 * r + 1 and r <= 2 * v + 1, (pair, pset, kind, regime, v, r)
    assert all(CT.bound(v) <= 12 for p in rec for s in rec[p] for k in rec[p][s] for v in rec[p][s][k].values())


def test_restatement_and_library_object_get_the_same_parameters(host_dev):
    for pset in CT.PARAMS:
        z = torch.tensor(CT.Z_ROWS, dtype=torch.float64)
        gc = CT.gpu_cost(_HostP, PAIR, pset, z)
        assert CT.host_cost(PAIR, pset, z).concentration == gc.concentration == CT.PARAMS[pset]
        assert torch.equal(gc.y_device(), z) and gc.desc().link == L.LINK_EXP and gc.is_native()


def test_host_cost_drives_the_oracle_unchanged():
    """the restatement is duck-typed like the oracle's costs: oracle.pls_oracle.PLS and train_pls take it"""
    from oracle import pls_oracle as O

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(40, 1, generator=g) * 2 - 1
        zi = x[:6].clone()
        y = torch.exp(x[:, 0]) * torch._standard_gamma(torch.full((40,), 3.0), generator=g) / 3.0
        ob = O.OrthonormalBasis(O.RBFARDKernel(torch.tensor([0.4]), 1.0), zi, x, 1e-2)
        oc = CT.GammaHostCost(torch.log(y), CT.ExpLink(), 3.0)
        u = 0.1 * torch.randn(ob.approximation_dimension, 5, generator=g)
        f = ob.calculate_untransformed_train_prediction_samples(u)
        assert torch.allclose(oc._autograd(f), oc.calculate_cost_derivative(f), rtol=1e-12, atol=1e-14)
        out, energies = O.train_pls(O.PLS(ob, oc), u.clone(), 5, 1e-3, 1e9, noises=[torch.zeros_like(u)] * 5)
        assert len(energies) == 5 and energies[-1] < energies[0] and torch.isfinite(out).all()
    finally:
        torch.set_default_dtype(prev)


# ---- the selector problems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_the_selector_problems_run_through_the_regimes(pset):
    """the lookup answers for the pair and for no other; the values drawn hold t near 0 and |t| > 100 with both signs, stay
    inside |f| <= 60 before the scaling by |c_n| <= 8, and every G is finite and survives the probe rows' scaling
    (SelectorProblem.expected asserts both)"""
    import cost_truth
    import ordinal_cost_truth

    assert truth_module(PAIR) is CT and truth_module("poisson/square") is cost_truth and truth_module("ordinal/identity") is ordinal_cost_truth
    with pytest.raises(KeyError):
        truth_module("gamma/identity")
    vals = truth_module(PAIR).SELECTOR_RANGE[PAIR](np.array([0.0, 60.0, 60.5, 1e9]))
    assert list(vals) == [True, True, False, False]
    ex = SelectorProblem(PAIR, 17, 333, 600, "head", seed=1, pset=pset)
    f, z = ex.f(), ex.y
    assert set(z.tolist()) == set(CT.Z_ROWS) and (z.abs() <= 30).all()
    assert (f.abs() <= 8 * 60 * (1 + 2.0 ** -4)).all()  # (|c_n| in [1/8, 8], the jiggle up to 1 + 2^-4)
    t = z[:, None] - f
    assert (t.abs() < 0.5).any() and (t > 100).any() and (t < -100).any() and t.abs().max() <= 541
    g = torch.as_tensor(CT.host_eval(PAIR, pset, "deriv_reference", z.numpy(), f.numpy()))
    assert torch.isfinite(g).all() and (g <= CT.PARAMS[pset]).all() and (g > 0).any() and (g < -1e40).any()
    want, probe, tol = ex.expected(g)
    assert torch.isfinite(want).all() and torch.isfinite(tol).all() and probe.sum() == ex.mk - 1
    v = torch.as_tensor(CT.host_eval(PAIR, pset, "value", z.numpy(), f.numpy()))
    assert torch.isfinite(v).all() and (v >= CT.PARAMS[pset]).all()
