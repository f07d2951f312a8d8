"""CPU: the ordinal cost without a GPU -- the descriptor and its +inf padding, argument validation in the C ABI (every refusal
with its own message, before any HIP call), the Python-side refusals, nativeness, cutpoints_from_labels, the predictive
distribution against mpmath, the two metrics, the checkpoint key, the ABI version; and the truth of
tests/ordinal_cost_truth.py: its grid, the library's cost against the full negative log-likelihood and against
Bernoulli/sigmoid in mpmath, the derivative as the value's slope, the recorded errors of the host restatement
(tests/golden/ordinal_cost_reference_errors.json) against a fresh measurement, and the regimes the selector problems of the
route tests run through."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import ordinal_cost_truth as CT
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd import costs, link_functions, metrics
from step_fixtures import SelectorProblem

L = pkg._lib
INF = math.inf
PAIR = "ordinal/identity"


class _HostP:
    """what tests/ordinal_cost_truth.py needs of the GPU tests' package fixture to build the library's cost object"""
    costs, links = costs, link_functions


def _cost(cutpoints=(-1.0, 0.5, 2.0), link=None, y=None):
    y = torch.tensor([0.0, 1.0, 2.0]) if y is None else y
    return costs.OrdinalCost(y, link or link_functions.IdentityLinkFunction(), cutpoints=list(cutpoints))


def _desc(p, link=None):
    d = L.CostDesc()
    d.cost, d.link, d.deriv_mode = L.COST_ORDINAL, L.LINK_IDENTITY if link is None else link, L.DERIV_REFERENCE
    for i in range(4):
        d.p[i] = p[i]
    d.jitter = 1e-10
    return d


def test_ids_exports_and_abi():
    assert L.COST_ORDINAL == 9
    assert L.ABI_VERSION == 7 and L.load().pls_abi_version() == 7
    assert pkg.OrdinalCost is costs.OrdinalCost and "OrdinalCost" in costs.__all__ and "OrdinalCost" in pkg.__all__


def test_descriptor_fields_and_the_inf_padding():
    for cut, want in (((0.25,), [0.25, INF, INF, INF]), ((-1.0, 0.5), [-1.0, 0.5, INF, INF]),
                      ((-1.0, 0.5, 2.0), [-1.0, 0.5, 2.0, INF]), ((-1.5, -0.25, 0.5, 2.0), [-1.5, -0.25, 0.5, 2.0])):
        c = _cost(cut, y=torch.tensor([0.0, 1.0]))
        assert c.observation_noise is None and c.cutpoints == tuple(cut) and c.number_of_categories == len(cut) + 1
        assert c._params() == tuple(want)
        for fa, mode in ((False, L.DERIV_REFERENCE), (True, L.DERIV_AUTOGRAD)):
            d = c.desc(force_autograd=fa)
            assert (d.cost, d.link, d.deriv_mode) == (L.COST_ORDINAL, L.LINK_IDENTITY, mode)
            assert list(d.p) == want


REFUSALS = [
    ((INF, INF, INF, INF), None, b"finite first cutpoint"),
    ((-INF, 0.0, INF, INF), None, b"finite first cutpoint"),
    ((math.nan, 0.0, INF, INF), None, b"is NaN"),
    ((0.0, math.nan, INF, INF), None, b"is NaN"),
    ((0.0, 1.0, 2.0, math.nan), None, b"is NaN"),
    ((0.0, 0.0, INF, INF), None, b"strictly increasing"),
    ((0.0, 1.0, 0.5, INF), None, b"strictly increasing"),
    ((0.0, 1.0, 2.0, -3.0), None, b"strictly increasing"),
    ((0.0, INF, 2.0, INF), None, b"after an infinite one"),
    ((0.0, 1.0, INF, 5.0), None, b"after an infinite one"),
    ((0.0, 1.0, -INF, INF), None, b"is -inf"),
    ((0.0, 1.0, INF, INF), L.LINK_SIGMOID, b"identity link"),
    ((0.0, 1.0, INF, INF), L.LINK_PROBIT, b"identity link"),
    ((0.0, 1.0, INF, INF), L.LINK_SQUARE, b"identity link"),
    ((0.0, 1.0, INF, INF), L.LINK_EXP, b"identity link"),
]


@pytest.mark.parametrize("p,link,word", REFUSALS)
def test_a_bad_descriptor_fails_before_any_hip_call(p, link, word):
    """(the pointers are not device memory: a kernel launched on them would fault, a refusal returns first)"""
    lib = L.load()
    d = _desc(p, link)
    assert lib.pls_cost_derivative(d, 8, 1, 8, 1, 1, 8, 1, None) == 1
    assert word in lib.pls_last_error() and b"ordinal" in lib.pls_last_error()
    assert lib.pls_cost_value(d, 8, 1, 8, 1, 1, 8, None, 0, None) == 1
    assert word in lib.pls_last_error() and b"ordinal" in lib.pls_last_error()


def test_the_new_id_passes_validation():
    """cost id 9 is known and 8 is not: validation goes on to the pointers (all NULL here, so no HIP call follows)"""
    lib = L.load()
    for p in ((0.0, INF, INF, INF), (-0.001, 0.002, INF, INF), (-1.5, -0.25, 0.5, 2.0)):
        assert lib.pls_cost_derivative(_desc(p), None, 1, None, 1, 1, None, 1, None) == 1
        assert b"NULL" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error() and b"ordinal" not in lib.pls_last_error()
    bad = _desc((0.0, INF, INF, INF))
    for kind in (6, 8, 10):
        bad.cost = kind
        assert lib.pls_cost_derivative(bad, 8, 1, 8, 1, 1, 8, 1, None) == 1 and b"unknown cost" in lib.pls_last_error()


def test_python_side_refusals():
    ident = link_functions.IdentityLinkFunction()
    y = torch.tensor([0.0, 1.0])
    with pytest.raises(ValueError, match="5 categories"):
        costs.OrdinalCost(y, ident, cutpoints=[-2.0, -1.0, 0.0, 1.0, 2.0])  # six categories
    with pytest.raises(ValueError, match="strictly increasing"):
        costs.OrdinalCost(y, ident, cutpoints=[0.5, -1.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        costs.OrdinalCost(y, ident, cutpoints=[0.5, 0.5])
    with pytest.raises(ValueError, match="finite"):
        costs.OrdinalCost(y, ident, cutpoints=[0.5, INF])
    with pytest.raises(ValueError, match="at least one"):
        costs.OrdinalCost(y, ident, cutpoints=[])
    for labels in ([0.0, 3.0], [-1.0, 0.0], [0.5, 1.0], [math.nan, 1.0]):
        with pytest.raises(ValueError, match=r"integer in \[0, 2\]"):
            costs.OrdinalCost(torch.tensor(labels), ident, cutpoints=[-1.0, 1.0])
    assert costs.OrdinalCost(torch.tensor([0, 2, 1]), ident, cutpoints=[-1.0, 1.0]).number_of_categories == 3  # integer dtype
    c = _cost()
    with pytest.raises(ValueError, match="strictly increasing"):
        c.cutpoints = [1.0, 0.0]
    assert c.cutpoints == (-1.0, 0.5, 2.0)


def test_is_native_unless_a_subclass_brings_its_own_torch_code():
    assert _cost().is_native()

    class Mine(costs.OrdinalCost):
        def calculate_cost(self, f):
            return f.sum(0)

    assert not Mine(torch.zeros(2), link_functions.IdentityLinkFunction(), cutpoints=[0.0]).is_native()


def test_cutpoints_from_labels_on_a_hand_computed_example():
    """counts 2, 1, 3 -> smoothed 2.5, 1.5, 3.5 of 7.5: cumulative 1/3 and 8/15, logits log(1/2) and log(8/7)"""
    y = torch.tensor([0, 0, 1, 2, 2, 2])
    got = costs.OrdinalCost.cutpoints_from_labels(y)
    assert len(got) == 2 and abs(got[0] - math.log(0.5)) < 1e-15 and abs(got[1] - math.log(8.0 / 7.0)) < 1e-15
    # an empty top category: counts 2, 1, 3, 0 -> 2.5, 1.5, 3.5, 0.5 of 8
    got = costs.OrdinalCost.cutpoints_from_labels(y.double(), num_categories=4)
    want = [math.log(2.5 / 5.5), math.log(4.0 / 4.0), math.log(7.5 / 0.5)]
    assert len(got) == 3 and all(abs(a - b) < 1e-14 for a, b in zip(got, want)) and got[0] < got[1] < got[2]
    # a latent at 0 reproduces the smoothed marginal frequencies
    c = costs.OrdinalCost(y, link_functions.IdentityLinkFunction(), cutpoints=costs.OrdinalCost.cutpoints_from_labels(y))
    probs = c.predict(torch.zeros(1, 3, dtype=torch.float64)).probs[0]
    assert torch.allclose(probs, torch.tensor([2.5, 1.5, 3.5], dtype=torch.float64) / 7.5, rtol=1e-14)
    for bad, k in ((torch.tensor([0, 5]), None), (torch.tensor([0, 0]), None), (torch.tensor([0, 3]), 3), (torch.tensor([0.5, 1.0]), None)):
        with pytest.raises(ValueError):
            costs.OrdinalCost.cutpoints_from_labels(bad, k)


@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_predict_against_mpmath_probabilities(pset):
    """per particle the product form against mpmath, at |f| = 40 too, relative: 8 x 2^-53 (three factors of <= 1 ulp and two
    products) plus 2^-53 |f - b| per sigmoid -- t = f - b is rounded once, and a relative rounding of t moves sigma(t) by up to
    |t| of it in its tail.  (As a difference of two cumulative probabilities the narrow category of set b would lose eleven
    bits everywhere.)  Rows sum to 1."""
    k = CT.categories(pset)
    cut = list(CT.PARAMS[pset])[:k - 1]
    c = costs.OrdinalCost(torch.arange(k), link_functions.IdentityLinkFunction(), cutpoints=cut)
    fs = [-40.0, -7.5, -1.0, -0.25, 0.0, 0.0005, 0.3, 1.0, 2.0, 6.0, 40.0]
    per = c.category_probabilities(torch.tensor(fs, dtype=torch.float64))
    assert per.shape == (len(fs), k)
    for a, f in enumerate(fs):
        want = CT.probabilities(CT.PARAMS[pset], f)
        for b in range(k):
            slack = sum(abs(f - c) for c in CT.cuts(pset, b) if math.isfinite(c))
            assert abs(mp.mpf(float(per[a, b])) - want[b]) <= (8 + slack) * CT.U * want[b], (pset, f, b, float(per[a, b]), want[b])
    assert ((per.sum(1) - 1).abs() <= 4 * 2.0 ** -52).all()
    samples = torch.tensor(fs + fs[::-1], dtype=torch.float64).reshape(2, len(fs))  # two test points, 11 particles each
    dist = c.predict(samples)
    assert isinstance(dist, torch.distributions.Categorical) and dist.probs.shape == (2, k)
    want = torch.tensor([float(sum(CT.probabilities(CT.PARAMS[pset], f)[b] for f in fs) / len(fs)) for b in range(k)], dtype=torch.float64)
    assert torch.allclose(dist.probs[0], want, rtol=1e-14, atol=0) and torch.allclose(dist.probs[1], want, rtol=1e-14, atol=0)
    assert ((dist.probs.sum(1) - 1).abs() <= 4 * 2.0 ** -52).all()


def test_the_two_metrics_of_a_categorical_prediction():
    probs = torch.tensor([[0.5, 0.25, 0.25], [0.125, 0.125, 0.75]], dtype=torch.float64)
    dist = torch.distributions.Categorical(probs=probs)
    y = torch.tensor([1.0, 2.0])
    point = metrics._point(dist)
    assert torch.equal(point, torch.tensor([0.75, 1.625], dtype=torch.float64))  # the expected category index
    assert metrics.calculate_mae(dist, y) == (0.25 + 0.375) / 2
    assert metrics.calculate_mse(dist, y) == (0.25 ** 2 + 0.375 ** 2) / 2
    assert abs(metrics.calculate_nll(dist, y) - (-(math.log(0.25) + math.log(0.75)) / 2)) < 1e-15
    assert abs(metrics.calculate_nll(dist, torch.tensor([1, 2])) - metrics.calculate_nll(dist, y)) == 0


def test_checkpoint_round_trips_the_cutpoints(tmp_path):
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    class Stub:
        def __init__(self, cost):
            self.cost, self.basis = cost, None
        observation_noise = property(lambda s: s.cost.observation_noise, lambda s, v: setattr(s.cost, "observation_noise", v))

    path = str(tmp_path / "ordinal.pt")
    u = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    save_pls(Stub(_cost((-1.0 / 3.0, 0.5, 2.0))), u, path, best_lr=1e-3, number_of_epochs=4)
    state = torch.load(path)
    assert state["cutpoints"] == [-1.0 / 3.0, 0.5, 2.0] and state["observation_noise"] is None
    assert "dispersion" not in state and "precision" not in state

    class Plain:
        basis = None
        cost = costs.PoissonCost(torch.zeros(2), link_functions.SquareLinkFunction())
        observation_noise = None

    save_pls(Plain(), torch.zeros(2, 2), str(tmp_path / "p.pt"))
    assert "cutpoints" not in torch.load(str(tmp_path / "p.pt"))
    if not torch.cuda.is_available():
        return  # (load_pls puts the particles on the device: tests/test_gpu_family_cost_train.py loads)
    other = Stub(_cost((0.0, 9.0)))
    _, got, lr, ep = load_pls(other, path)
    assert other.cost.cutpoints == (-1.0 / 3.0, 0.5, 2.0) and torch.equal(got.cpu(), u) and (lr, ep) == (1e-3, 4)


# ---- the truth ------------------------------------------------------------------------------------------------------------------
def _library_cuts(pset, label):
    """(lo, hi) of a label as the header maps it onto the descriptor the library's class builds for the parameter set: the
    truth's own mapping (CT.cuts) must be this one"""
    k = CT.categories(pset)
    p = costs.OrdinalCost(torch.arange(k), link_functions.IdentityLinkFunction(), cutpoints=list(CT.PARAMS[pset])[:k - 1])._params()
    assert p == tuple(CT.PARAMS[pset])
    b = (-INF,) + p + (INF,)
    return b[int(label)], b[int(label) + 1]


@pytest.mark.parametrize("pair,pset", CT.cells())
def test_grid_layout_and_regimes(pair, pset):
    y, f, regimes = CT.grid(pair, pset)
    n, j = f.shape
    k = CT.categories(pset)
    assert k == {"a": 5, "b": 3}[pset]
    assert n % 2 == 1 and j % 2 == 1 and y.shape == (n,) and len(regimes) == j
    assert set(y) == set(float(v) for v in range(k))
    assert set(regimes) == {"bulk", "cut", "root", "lo_tail", "hi_tail", "far", "zero"}
    col = lambda name: f[:, [b for b, r in enumerate(regimes) if r == name]]  # noqa: E731
    assert (np.abs(col("bulk")) <= 3).all() and (col("zero") == 0).any() and np.signbit(f[f == 0]).any()
    assert (np.abs(col("zero")) < 2.3e-308).all() and (col("zero") != 0).any()
    assert col("hi_tail").min() == 30 and col("hi_tail").max() == 700 and col("lo_tail").max() == -30 and col("lo_tail").min() == -700
    assert {745.0, -745.0, 1e10, -1e10, 1e150, -1e150, 1e300, -1e300} == set(col("far").ravel())
    cut, root = col("cut"), col("root")
    for a, yy in enumerate(y):
        lo, hi = CT.cuts(pset, yy)
        assert (lo, hi) == _library_cuts(pset, yy)
        flo, fhi = CT.finite_cuts(pset, yy)
        assert math.isfinite(flo) and math.isfinite(fhi) and flo < fhi and {flo, fhi} & {lo, hi}
        for c in (flo, fhi):  # both sides of each cutpoint, from 2^-8 down to 2^-50
            d = cut[a] - c
            near = d[np.abs(d) <= 2.0 ** -8]
            assert (near > 0).any() and (near < 0).any() and np.abs(near).min() <= 2.0 ** -49 and np.abs(near).max() == 2.0 ** -8
        if CT.interior(pset, yy):
            rel = (root[a] - (lo + hi) / 2) / (hi - lo)
            assert np.abs(rel).min() < 2.0 ** -49 and np.abs(rel).max() <= 2.0 ** -7 and (rel > 0).any() and (rel < 0).any()
        else:
            assert set(root[a]) == {(-1.0 if lo == -INF else 1.0) * v for v in (8, 20, 30, 40, 50)}


def test_the_cost_is_the_full_nll_without_its_constant():
    """-log[sigma(hi - f) - sigma(lo - f)] = softplus(f - hi) + softplus(lo - f) - log(1 - e^-(hi - lo)), in mpmath on the grid
    (wherever e^f can be formed: |f| <= 700) and on a plain grid of f"""
    with mp.workdps(400):  # (sigma(hi - f) - sigma(lo - f) cancels e^|f| / (hi - lo) of its digits: 310 of them at |f| = 700)
        for pset in CT.PARAMS:
            y, f, _ = CT.grid(PAIR, pset)
            for a in range(len(y)):
                lo, hi = _library_cuts(pset, float(y[a]))
                const = -mp.log(-mp.expm1(-(mp.mpf(hi) - mp.mpf(lo)))) if CT.interior(pset, float(y[a])) else mp.mpf(0)
                for v in list(f[a]) + [x / 4 for x in range(-60, 61)]:
                    if abs(v) > 1e5:
                        continue
                    cost = CT.ordinal_form(lo, hi, float(v))[0]
                    nll = CT.full_nll(lo, hi, float(v))
                    assert abs(nll - (cost + const)) <= mp.mpf(10) ** -60 * (abs(nll) + 1), (pset, y[a], v)
    # the ends: an edge label's own side underflows to 0, the other side is linear; the derivative is 0 / +-1
    v, d, _, _ = CT.ordinal_form(-INF, -1.5, -1e300)
    assert v == 0 and d == 0
    v, d, _, _ = CT.ordinal_form(-INF, -1.5, 1e300)
    assert v == mp.mpf(1e300) + mp.mpf(1.5) and d == 1
    v, d, _, _ = CT.ordinal_form(-0.001, 0.002, -1e300)
    assert v == mp.mpf(1e300) - mp.mpf(0.001) and d == -1


def test_two_categories_with_the_cutpoint_zero_are_bernoulli_sigmoid():
    """K = 2, b_1 = 0: label 1 costs softplus(-f) = -log sigma(f) and label 0 softplus(f) = -log(1 - sigma(f)); the
    derivative is sigma(f) - y -- Bernoulli/sigmoid without its clip"""
    b = (-INF,) + _cost((0.0,), y=torch.tensor([0.0, 1.0]))._params() + (INF,)  # (the library's descriptor for this model)
    assert b[:3] == (-INF, 0.0, INF)
    with mp.workdps(400):  # (1 - sigma(f) is formed as a difference: e^|f| of the digits cancel)
        for f in [x / 8 for x in range(-240, 241)] + [-700.0, 700.0]:
            fm = mp.mpf(f)
            p = 1 / (1 + mp.exp(-fm))
            for label, (lo, hi) in ((0, b[0:2]), (1, b[1:3])):
                v, d, _, _ = CT.ordinal_form(lo, hi, f)
                want = -mp.log(p) if label == 1 else -mp.log(1 - p)
                assert abs(v - want) <= mp.mpf(10) ** -60 * abs(want), (f, label)
                assert abs(d - (p - label)) <= mp.mpf(10) ** -60 * abs(d), (f, label)


def test_the_derivative_is_the_values_slope():
    with mp.workdps(130):
        for pair, pset in CT.cells():
            y, f, regimes = CT.grid(pair, pset)
            assert all(CT.cuts(pset, float(yy)) == _library_cuts(pset, float(yy)) for yy in y)
            for a in range(len(y)):
                for b in range(0, f.shape[1], 2):
                    yy, ff = float(y[a]), float(f[a, b])
                    if abs(ff) > 1e5:
                        continue
                    t, cu = CT.point_truth(pair, pset, "deriv_autograd", yy, ff)
                    assert t == CT.point_truth(pair, pset, "deriv_reference", yy, ff)[0] and -1 <= t <= 1
                    h = mp.mpf(2) ** -70 * abs(mp.mpf(ff)) if ff != 0 else mp.mpf(2) ** -1200
                    vp = CT.point_truth(pair, pset, "value", yy, mp.mpf(ff) + h)[0]
                    vm = CT.point_truth(pair, pset, "value", yy, mp.mpf(ff) - h)[0]
                    num = (vp - vm) / (2 * h)
                    tol = mp.mpf(2) ** -40 * cu / CT.U + (abs(vp) + 1) / h * mp.mpf(2) ** -400
                    assert abs(num - t) <= tol, (pair, pset, regimes[b], yy, ff, num, t)


def test_host_restatement_against_truth_matches_the_recorded_errors():
    """A fresh run of the restatement on the grid against the file: torch's vectorised exp / log differ by an ulp between CPU
    generations, so fresh and recorded must agree within a factor of two plus one unit (as tests/test_count_cost_host.py holds
    its restatement); no cell is a miss, and both derivative modes are the same numbers."""
    fresh, rec = CT.measure_reference(), CT.reference_errors()
    for pset in CT.PARAMS:  # (the restatement and the library's class are handed the same cutpoints)
        assert tuple(CT.host_cost(PAIR, pset, torch.zeros(1)).cutpoints) == CT.gpu_cost(_HostP, PAIR, pset, torch.zeros(1)).cutpoints
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
        y = torch.bucketize(2 * x[:, 0] + 0.3 * torch.randn(40, generator=g), torch.tensor([-1.0, 0.0, 1.0])).double()
        ob = O.OrthonormalBasis(O.RBFARDKernel(torch.tensor([0.4]), 1.0), z, x, 1e-2)
        oc = CT.OrdinalHostCost(y, O.IdentityLink(), costs.OrdinalCost.cutpoints_from_labels(y))
        u = 0.1 * torch.randn(ob.approximation_dimension, 5, generator=g)
        f = ob.calculate_untransformed_train_prediction_samples(u)
        assert torch.allclose(oc._autograd(f), oc.calculate_cost_derivative(f), rtol=1e-12, atol=1e-14)
        out, energies = O.train_pls(O.PLS(ob, oc), u.clone(), 5, 1e-2, 1e9, noises=[torch.zeros_like(u)] * 5)
        assert len(energies) == 5 and energies[-1] < energies[0] and torch.isfinite(out).all()
    finally:
        torch.set_default_dtype(prev)


def test_the_selector_problems_run_through_the_regimes():
    """the values drawn still hold |f| < 3 and |f| > 20, both signs, every label of the parameter set and a value >= 1e9;
    none lies where an edge label's derivative would fall between 2^-1000 and 0"""
    for pset in CT.PARAMS:
        ex = SelectorProblem(PAIR, 17, 333, 600, "head", seed=1, pset=pset)
        f = ex.f()
        assert (f.abs() < 3).any() and (f.abs() > 20).any() and (f > 0).any() and (f < 0).any()
        assert (f >= 1e9).any() and (f <= -1e9).any()
        assert set(ex.y.tolist()) == set(float(k) for k in range(CT.categories(pset)))
        a = f.abs()
        assert ((a <= 8 * 75 * (1 + 2.0 ** -4)) | (a >= 1e9 / 8)).all()  # (|c_n| in [1/8, 8], the jiggle up to 1 + 2^-4)
