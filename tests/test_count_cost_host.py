"""CPU: the negative-binomial cost and the exponential link without a GPU -- descriptors, argument validation in the C ABI,
nativeness, the predictive distribution, the checkpoint key, the ABI version; and the truth of tests/count_cost_truth.py: its
grid, the header's formula in mu against the softplus form in mpmath, the derivative as the value's slope, the recorded
errors of the host restatement (tests/golden/count_cost_reference_errors.json) against a fresh measurement, and the regimes the
selector problems of the route tests run through."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import count_cost_truth as CT
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd import costs, link_functions
from step_fixtures import SelectorProblem

L = pkg._lib


def _cost(r=0.7, link=None, y=None):
    return costs.NegativeBinomialCost(torch.tensor([0.0, 1.0, 3.0]) if y is None else y, link or link_functions.ExponentialLinkFunction(), r)


def test_ids_exports_and_abi():
    assert L.COST_NEGATIVE_BINOMIAL == 5 and L.LINK_EXP == 4 and L.LINK_EXP < 7
    assert L.ABI_VERSION == 7 and L.load().pls_abi_version() == 7
    assert pkg.NegativeBinomialCost is costs.NegativeBinomialCost and pkg.ExponentialLinkFunction is link_functions.ExponentialLinkFunction
    assert "NegativeBinomialCost" in costs.__all__ and "NegativeBinomialCost" in pkg.__all__ and "ExponentialLinkFunction" in pkg.__all__
    assert link_functions.ExponentialLinkFunction.kind == L.LINK_EXP


def test_descriptor_fields_in_both_modes():
    c = _cost(r=3.5)
    assert c.observation_noise is None and c._params() == (3.5, 0.0, 0.0, 0.0) and c.dispersion == 3.5
    for fa, mode in ((False, L.DERIV_REFERENCE), (True, L.DERIV_AUTOGRAD)):
        d = c.desc(force_autograd=fa)
        assert (d.cost, d.link, d.deriv_mode) == (L.COST_NEGATIVE_BINOMIAL, L.LINK_EXP, mode)
        assert list(d.p) == [3.5, 0.0, 0.0, 0.0] and d.jitter == 1e-10
    d = _cost(link=link_functions.SquareLinkFunction()).desc()
    assert (d.cost, d.link) == (L.COST_NEGATIVE_BINOMIAL, L.LINK_SQUARE)
    d = costs.GaussianCost(0.3, torch.zeros(3), link_functions.ExponentialLinkFunction()).desc()
    assert (d.cost, d.link) == (L.COST_GAUSSIAN, L.LINK_EXP)


@pytest.mark.parametrize("r", [0.0, -1.0, math.inf, math.nan])
def test_a_bad_dispersion_fails_before_any_hip_call(r):
    lib = L.load()
    d = _cost(r=r).desc()
    assert lib.pls_cost_derivative(d, 8, 1, 8, 1, 1, 8, 1, None) == 1
    assert b"dispersion" in lib.pls_last_error()
    assert lib.pls_cost_value(d, 8, 1, 8, 1, 1, 8, None, 0, None) == 1
    assert b"dispersion" in lib.pls_last_error()


def test_the_new_ids_pass_validation():
    """link id 4 and cost id 5 are known: validation goes on to the pointers (all NULL here, so no HIP call follows)"""
    lib = L.load()
    d = _cost().desc()
    assert lib.pls_cost_derivative(d, None, 1, None, 1, 1, None, 1, None) == 1
    assert b"NULL" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_link_transform(L.LINK_EXP, 0.0, None, 1, 1, 1, None, None, 1, None) == 1
    assert b"bad arguments" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    for cost, link, word in ((6, L.LINK_EXP, b"unknown cost"), (L.COST_NEGATIVE_BINOMIAL, 5, b"unknown link"), (L.COST_NEGATIVE_BINOMIAL, 7, b"unknown link")):
        bad = L.CostDesc()
        bad.cost, bad.link, bad.p[0] = cost, link, 1.0
        assert lib.pls_cost_derivative(bad, 8, 1, 8, 1, 1, 8, 1, None) == 1 and word in lib.pls_last_error()
    assert lib.pls_link_transform(5, 0.0, 8, 1, 1, 1, None, 8, 1, None) == 1 and b"unknown link" in lib.pls_last_error()


def test_is_native_unless_a_subclass_brings_its_own_torch_code():
    assert _cost().is_native()

    class Mine(costs.NegativeBinomialCost):
        def calculate_cost(self, f):
            return f.sum(0)

    assert not Mine(torch.zeros(2), link_functions.ExponentialLinkFunction(), 1.0).is_native()

    class TorchLink(link_functions.PLSLinkFunction):
        def transform(self, y):
            return y.exp()

    assert not _cost(link=TorchLink()).is_native()


def test_predict_returns_the_negative_binomial_with_the_samples_mean():
    g = torch.Generator().manual_seed(0)
    samples = torch.rand(5, 40, generator=g, dtype=torch.float64) * 9 + 0.1
    r = 2.5
    dist = _cost(r=r).predict(samples)
    assert isinstance(dist, torch.distributions.NegativeBinomial)
    mu = samples.mean(dim=1)
    assert torch.allclose(dist.mean, mu, rtol=1e-13) and torch.allclose(dist.variance, mu + mu * mu / r, rtol=1e-12)
    assert torch.equal(dist.total_count, torch.full((5,), r, dtype=torch.float64))


def test_checkpoint_round_trips_the_dispersion(tmp_path):
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    class Stub:
        def __init__(self, cost):
            self.cost, self.basis = cost, None
        observation_noise = property(lambda s: s.cost.observation_noise, lambda s, v: setattr(s.cost, "observation_noise", v))

    path = str(tmp_path / "nb.pt")
    u = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    save_pls(Stub(_cost(r=1.0 / 3.0)), u, path, best_lr=1e-3, number_of_epochs=4)
    state = torch.load(path)
    assert state["dispersion"] == 1.0 / 3.0 and state["observation_noise"] is None
    if not torch.cuda.is_available():
        return  # (load_pls puts the particles on the device: tests/test_gpu_family_cost_train.py loads)
    other = Stub(_cost(r=9.0))
    _, got, lr, ep = load_pls(other, path)
    assert other.cost.dispersion == 1.0 / 3.0 and torch.equal(got.cpu(), u) and (lr, ep) == (1e-3, 4)


def test_a_cost_without_a_dispersion_writes_no_such_key(tmp_path):
    from projected_langevin_sampling_amd.checkpoint import save_pls

    class Stub:
        basis = None
        cost = costs.PoissonCost(torch.zeros(2), link_functions.SquareLinkFunction())
        observation_noise = None

    path = str(tmp_path / "p.pt")
    save_pls(Stub(), torch.zeros(2, 2), path)
    assert "dispersion" not in torch.load(path)


# ---- the truth ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,pset", CT.cells())
def test_grid_layout_and_regimes(pair, pset):
    y, f, regimes = CT.grid(pair, pset)
    n, j = f.shape
    assert n % 2 == 1 and j % 2 == 1 and y.shape == (n,) and len(regimes) == j
    assert set(y) == {0.0, 1.0, 3.0, 25.0, 1e6, 0.5, 1.0 / 3.0}
    assert set(regimes) == {"bulk", "root", "lo_tail", "hi_tail", "far", "zero"}
    col = lambda name: f[:, [b for b, r in enumerate(regimes) if r == name]]  # noqa: E731
    assert (np.abs(col("bulk")) <= 3).all() and (col("zero") == 0).any() and np.signbit(f[f == 0]).any()
    assert (np.abs(col("zero")) < 2.3e-308).all() and (col("zero") != 0).any()
    assert col("hi_tail").min() == 30 and col("hi_tail").max() == 700 and col("lo_tail").max() == -30 and col("lo_tail").min() == -700
    assert {745.0, -745.0, 1e10, -1e10, 1e150, -1e150, 1e300, -1e300} == set(col("far").ravel())
    root = col("root")
    for a, yy in enumerate(y):
        if yy > 0:
            rel = np.abs(np.expm1(root[a] - math.log(yy)))
            assert rel.min() < 2.0 ** -49 and rel.max() < 2.0 ** -7 and (root[a] > math.log(yy)).any() and (root[a] < math.log(yy)).any()


def test_the_header_formula_is_the_softplus_form():
    """r log1p(mu / r) + y log1p(r / mu) and r (mu - y) / (mu (r + mu)) mu against r softplus(t) + y softplus(-t) and
    r sigma(t) - y sigma(-t), in mpmath, wherever mu = e^f can be formed at 50 digits"""
    for pset in CT.PARAMS:
        (r,) = CT.PARAMS[pset]["negative_binomial"]
        y, f, _ = CT.grid("negative_binomial/exp", pset)
        for a in range(len(y)):
            for v in f[a]:
                if abs(v) > 1e5:
                    continue
                v1, d1 = CT.nb_mu_form(r, float(y[a]), float(v))
                v2, d2, sa, sb = CT.nb_softplus_form(r, float(y[a]), float(v))
                assert abs(v1 - v2) <= mp.mpf(10) ** -44 * (abs(v2) + 1), (r, y[a], v)
                assert abs(d1 - d2) <= mp.mpf(10) ** -44 * (sa + sb), (r, y[a], v)
    # y = 0: the second term is exactly 0; the value's ends are r t and -y t
    assert CT.nb_softplus_form(0.7, 0.0, -1e300)[0] == 0
    v, d, _, _ = CT.nb_softplus_form(50.0, 3.0, 1e300)
    assert abs(v / (50 * (mp.mpf(1e300) - mp.log(50))) - 1) < mp.mpf(10) ** -45 and d == 50
    v, d, _, _ = CT.nb_softplus_form(50.0, 3.0, -1e300)
    assert abs(v / (3 * (mp.mpf(1e300) + mp.log(50))) - 1) < mp.mpf(10) ** -45 and d == -3


def test_the_derivative_is_the_values_slope():
    with mp.workdps(130):
        for pair, pset in CT.cells():
            y, f, regimes = CT.grid(pair, pset)
            for a in range(len(y)):
                for b in range(0, f.shape[1], 2):
                    yy, ff = float(y[a]), float(f[a, b])
                    if abs(ff) > 1e5:
                        continue
                    t, cu = CT.point_truth(pair, pset, "deriv_autograd", yy, ff)
                    cu = cu[0] if isinstance(cu, tuple) else cu
                    assert t == CT.point_truth(pair, pset, "deriv_reference", yy, ff)[0]
                    h = mp.mpf(2) ** -70 * abs(mp.mpf(ff)) if ff != 0 else mp.mpf(2) ** -1200
                    vp = CT.point_truth(pair, pset, "value", yy, mp.mpf(ff) + h)[0]
                    vm = CT.point_truth(pair, pset, "value", yy, mp.mpf(ff) - h)[0]
                    num = (vp - vm) / (2 * h)
                    tol = mp.mpf(2) ** -40 * cu / CT.U + (abs(vp) + 1) / h * mp.mpf(2) ** -400
                    assert abs(num - t) <= tol, (pair, pset, regimes[b], yy, ff, num, t)


def test_host_restatement_against_truth_matches_the_recorded_errors():
    """A fresh run of the restatement on the grid against the file: torch's vectorised exp / log differ by an ulp between CPU
    generations, so fresh and recorded must agree within a factor of two plus one unit (as tests/test_cost_truth_host.py holds
    the oracle's); no cell is a miss, and both derivative modes are the same numbers."""
    fresh, rec = CT.measure_reference(), CT.reference_errors()
    assert {(p, s) for p in rec for s in rec[p]} == set(CT.cells())
    for pair, pset in CT.cells():
        assert set(fresh[pair][pset]) == set(rec[pair][pset]) == set(CT.KINDS)
        assert rec[pair][pset]["deriv_reference"] == rec[pair][pset]["deriv_autograd"]
        for kind, cells in fresh[pair][pset].items():
            assert set(cells) == set(rec[pair][pset][kind]) == set(CT.grid(pair, pset)[2])
            for regime, v in cells.items():
                r = rec[pair][pset][kind][regime]
                assert r != "inf" and math.isfinite(v) and r < CT.T.ORACLE_MISS, (pair, pset, kind, regime, v, r)
                assert v <= 2 * r + 1 and r <= 2 * v + 1, (pair, pset, kind, regime, v, r)
    assert all(CT.bound(v) <= 4e3 for p in rec for s in rec[p] for k in rec[p][s] for v in rec[p][s][k].values())


def test_host_cost_drives_the_oracle_unchanged():
    """the restatement is duck-typed like the oracle's costs: oracle.pls_oracle.PLS and train_pls take it"""
    from oracle import pls_oracle as O

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(40, 1, generator=g) * 2 - 1
        z = x[:6].clone()
        y = torch.poisson(torch.exp(1 + x[:, 0]), generator=g)
        ob = O.OrthonormalBasis(O.RBFARDKernel(torch.tensor([0.4]), 1.0), z, x, 1e-2)
        oc = CT.NegativeBinomialHostCost(y, CT.ExpLink(), 2.0)
        u = 0.1 * torch.randn(ob.approximation_dimension, 5, generator=g)
        f = ob.calculate_untransformed_train_prediction_samples(u)
        assert torch.allclose(oc._autograd(f), oc.calculate_cost_derivative(f), rtol=1e-12, atol=1e-14)
        out, energies = O.train_pls(O.PLS(ob, oc), u.clone(), 5, 1e-4, 1e9, noises=[torch.zeros_like(u)] * 5)
        assert len(energies) == 5 and energies[-1] < energies[0] and torch.isfinite(out).all()
    finally:
        torch.set_default_dtype(prev)


def test_the_selector_problems_run_through_the_regimes():
    for pair in CT.PAIRS:
        ex = SelectorProblem(pair, 17, 333, 600, "head", seed=1)
        f = ex.f()
        assert (f.abs() < 3).any() and (f.abs() > 20).any() and (f > 0).any() and (f < 0).any()
        assert set(ex.y.tolist()) == {0.0, 1.0, 3.0, 25.0, 1e6, 0.5, 1.0 / 3.0}
    assert (SelectorProblem("negative_binomial/exp", 17, 333, 600, "head", seed=1).f().abs() > 1e9).any()
