"""The selector problems of tests/step_fixtures.py for the ordinal pair of tests/ordinal_cost_truth.py: the same construction
(a probe row of a step shows G[n_k, :] bit for bit), with the carrier values, the labels, the library's cost object and the
mpmath truth taken from ordinal_cost_truth instead of cost_truth -- the four places the base classes reach into cost_truth by
pair name.  And the Winograd case of tests/test_gpu_cost_routes.py bound to any such fixtures, once, for the cost-route tests
that need it."""
import types

import mpmath as mp
import numpy as np
import torch

import ordinal_cost_truth as CT
from step_fixtures import SelectorIpbProblem, SelectorProblem

# Carrier values F = c_n V_j with |c_n| <= 8 and a jiggle of up to 1 + 2^-4.  The probe rows must neither overflow nor land
# between 2^-1000 and 0 after the scaling by eta 2^p >= 2^-23 (SelectorProblem.expected):
#   ordinal/identity: G lies in (-1, 1); in an edge label's own tail it is +-sigma(-|F - b|) ~ e^-|F|, fine down to
#     |F| = 640 (e^-640 = 2^-923) and exactly 0 from |F| = 1e9 on (e^-|F| underflows from 745), so |f| <= 75 or |f| >= 1e9
#     (the grid's +-1e10: value and derivative in their linear ends), as for the negative binomial
SELECTOR_RANGE = {"ordinal/identity": lambda a: (a <= 75) | ((a >= 1e9) & (a <= 1e30))}


def selector_values(pair, pset="a"):
    y, f, _ = CT.grid(pair, pset)
    a = np.abs(f)
    keep = np.isfinite(f) & (a >= 1e-30) & SELECTOR_RANGE[pair](a)
    return np.unique(f[keep]), y


class _OrdinalMixin:
    def _ordinal_values(self, seed):
        """v, y and U[k0] again, from the ordinal grid (the base constructor, which knows the pairs of cost_truth only, has
        drawn them from its fall-through grid); everything else of the construction stays"""
        g = torch.Generator().manual_seed(seed + 4242)
        j, n = self.j, self.n
        vals, ys = selector_values(self.pair, self.pset)
        pick = torch.as_tensor(vals)[torch.randint(0, len(vals), (j,), generator=g)]
        jiggle = 1 + (torch.rand(j, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -3
        third = torch.arange(j) % 3
        self.v = torch.where(third == 0, pick, torch.where(third == 1, pick * jiggle, 1.5 * torch.randn(j, generator=g, dtype=torch.float64)))
        self.v[self.v == 0] = 0.75
        self.y = torch.as_tensor(ys)[torch.randint(0, len(ys), (n,), generator=g)]
        self.u = torch.zeros(self.mk, j, dtype=torch.float64)
        self.u[self.k0] = self.v
        self._check()

    def cost(self, P, force_autograd=False):
        cost = CT.gpu_cost(P, self.pair, self.pset, self.y)
        if force_autograd:
            plain = cost.desc
            cost.desc = lambda force_autograd=False: plain(force_autograd=True)
        return cost

    def values_direct(self, P, cols=None):
        f = self.f(cols)
        out = torch.empty_like(f)
        for yy in torch.unique(self.y).tolist():
            rows = (self.y == yy).nonzero().flatten()
            cost = CT.gpu_cost(P, self.pair, self.pset, torch.tensor([yy], dtype=torch.float64))
            out[rows] = cost.calculate_cost(f[rows].reshape(1, -1).cuda()).cpu().reshape(len(rows), -1)
        return out

    def energy_truth(self, cols):
        f = self.f(cols)
        want, mag, units = [], [], []
        for b, col in enumerate(torch.as_tensor(cols).tolist()):
            tot, ab, un = mp.mpf(0), mp.mpf(0), mp.mpf(0)
            for a in range(self.n):
                t, cu = CT.point_truth(self.pair, self.pset, "value", float(self.y[a]), float(f[a, b]))
                tot, ab, un = tot + t, ab + abs(t), un + max(cu, abs(t) * mp.mpf(2) ** -52)
            want.append(float(tot + mp.mpf(self.prior_energy(col))))
            mag.append(float(ab))
            units.append(float(un))
        return tuple(torch.tensor(x, dtype=torch.float64) for x in (want, mag, units))


class OrdinalSelectorProblem(_OrdinalMixin, SelectorProblem):
    def __init__(self, pair, mk, n, j, placement="head", seed=0, pset="a", k0=None):
        assert pair in CT.PAIRS
        super().__init__(pair, mk, n, j, placement, seed, pset, k0)
        self._ordinal_values(seed)


class OrdinalSelectorIpbProblem(_OrdinalMixin, SelectorIpbProblem):
    def __init__(self, pair, m, n, j, placement="head", seed=0, pset="a"):
        assert pair in CT.PAIRS
        super().__init__(pair, m, n, j, placement, seed, pset)
        self._ordinal_values(seed)
        self.u = self.u * (self.d * self.d)[:, None]  # exact: powers of four
        self.s = self.u / self.d[:, None]
        self.state = self.u


def energy_check(P, ex, gb, cost, e, what, cols=None, truth=False, particle_energy=True):
    """tests/test_gpu_cost_routes.py energy_check with the bounds of ordinal_cost_truth: the energy by-product and
    fused_particle_energy against fsum of the element-wise entry's values plus the exact prior (N roundings), and, ``truth``,
    on three columns against fsum of the mpmath values (N roundings, and per element the pair's bound in its unit)"""
    got = [("by-product", e)]
    if particle_energy:
        got.append(("fused_particle_energy", gb.fused_particle_energy(cost, ex.u.cuda(), force_generic=True)))
    idx = torch.arange(ex.j) if cols is None else torch.as_tensor(cols)
    want, tol = ex.energy_direct(P, idx)
    for name, en in got:
        err = (en.cpu()[idx] - want).abs()
        assert (err <= tol).all(), f"{what}: energy {name} off by {(err / tol).max().item():.2f} x its summation bound"
    if truth:
        idx = torch.unique(torch.linspace(0, ex.j - 1, 3).long())
        want, mag, units = ex.energy_truth(idx)
        b = max(CT.bound(v) for v in CT.reference_errors()[ex.pair][ex.pset]["value"].values())
        tol = (ex.n + 2) * 2.0 ** -53 * (mag + want.abs()) + b * units
        for name, en in got:
            err = (en.cpu()[idx] - want).abs()
            print(f"{what} energy {name}: max error / bound {(err / tol).max().item():.3f}")
            assert (err <= tol).all(), f"{what}: energy {name} off by {(err / tol).max().item():.2f} x its bound"


def bind_winograd_case(problem_class, check, name):
    """The Winograd case of tests/test_gpu_cost_routes.py, word for word, with the two names through which it reaches
    cost_truth (the problem class and the energy check) bound to another pair's fixtures: a copy of the function over its own
    globals, the module it comes from is left as it is.  ``check``: an energy_check of this module's signature."""
    import test_gpu_cost_routes as R

    def bound_check(P, ex, gb, cost, e, what, cols=None, gauss_fma=False, truth=False, particle_energy=True):
        assert not gauss_fma
        check(P, ex, gb, cost, e, what, cols, truth, particle_energy)

    return types.FunctionType(R.winograd_case.__code__, {**vars(R), "SelectorProblem": problem_class, "energy_check": bound_check},
                              name, R.winograd_case.__defaults__, R.winograd_case.__closure__)
