"""Loader for tests/golden/oracle_step_vectors.npz (written by tests/golden/make_oracle_step_vectors.py): the frozen
Langevin step.  Builds the oracle's objects -- and, for the GPU tests, the library's -- from the stored inputs."""
import math
import os

import numpy as np
import pytest
import torch

from cost_families import truth_module
from oracle import pls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = ["gaussian/identity", "poisson/square", "bernoulli/sigmoid", "bernoulli/probit", "student_t/identity",
         "multimodal/identity"]
TAGS = ["a", "c1"]
BASES = ["onb", "ipb"]


def load():
    return dict(np.load(os.path.join(HERE, "golden", "oracle_step_vectors.npz")))


def t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def rel(got, want):
    got, want = t(got.detach().cpu() if isinstance(got, torch.Tensor) else got), t(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def oracle_costs(v, tag):
    y, yc, yb = t(v[f"{tag}/y"]), t(v[f"{tag}/y_count"]), t(v[f"{tag}/y_bin"])
    return {
        "gaussian/identity": O.GaussianCost(0.3, y, O.IdentityLink()),
        "poisson/square": O.PoissonCost(yc, O.SquareLink()),
        "bernoulli/sigmoid": O.BernoulliCost(yb, O.SigmoidLink()),
        "bernoulli/probit": O.BernoulliCost(yb, O.ProbitLink()),
        "student_t/identity": O.StudentTCost(3.0, y, O.IdentityLink(), 0.7),
        "multimodal/identity": O.MultiModalCost(0.7, 1.5, 0.3, y, O.IdentityLink()),
    }


def oracle_bases(v, tag):
    kern = O.RBFARDKernel(t(v[f"{tag}/ls"]), float(v[f"{tag}/scale"]))
    x, z, y = t(v[f"{tag}/x"]), t(v[f"{tag}/z"]), t(v[f"{tag}/y"])
    onb = O.OrthonormalBasis(kern, z, x, float(v[f"{tag}/threshold"]),
                             spectrum=(t(v[f"{tag}/spectrum_values"]), t(v[f"{tag}/spectrum_vectors"])))
    ipb = O.InducingPointBasis(kern, z, y[: z.shape[0]], x)
    return {"onb": onb, "ipb": ipb}


def gpu_costs(P, v, tag):
    y, yc, yb = t(v[f"{tag}/y"]), t(v[f"{tag}/y_count"]), t(v[f"{tag}/y_bin"])
    C, Lk = P.costs, P.links
    return {
        "gaussian/identity": C.GaussianCost(0.3, y, Lk.IdentityLinkFunction()),
        "poisson/square": C.PoissonCost(yc, Lk.SquareLinkFunction()),
        "bernoulli/sigmoid": C.BernoulliCost(yb, Lk.SigmoidLinkFunction()),
        "bernoulli/probit": C.BernoulliCost(yb, Lk.ProbitLinkFunction()),
        "student_t/identity": C.StudentTCost(3.0, y, Lk.IdentityLinkFunction(), 0.7),
        "multimodal/identity": C.MultiModalCost(0.7, 1.5, 0.3, y, Lk.IdentityLinkFunction()),
    }


def gpu_bases(P, v, tag):
    x, z, y = t(v[f"{tag}/x"]), t(v[f"{tag}/z"]), t(v[f"{tag}/y"])
    kern = P.pkg.PLSKernel(P.pkg.ARDKernel(t(v[f"{tag}/ls"]), float(v[f"{tag}/scale"])), z)
    onb = P.basis.OrthonormalBasis(kern, z, x, float(v[f"{tag}/threshold"]),
                                   spectrum=(t(v[f"{tag}/spectrum_values"]), t(v[f"{tag}/spectrum_vectors"])), verbose=False)
    ipb = P.basis.InducingPointBasis(kern, z, y[: z.shape[0]], x)
    return {"onb": onb, "ipb": ipb}


# ---- exact problems: integer operands on which every ONB step route is exact ------------------------------------------------
# A (M_k x N), U, y and the injected noise are small integers, the eigenvalues powers of two, the Gaussian variance 1/4 and the
# step size 2^-21 (sqrt(2 eta) = 2^-10).  Every intermediate a route forms -- F = A^T U, G = 4 (F - y), the split-K slabs of
# D = A G, Winograd's S1..S4, T1..T4 and seven products, the fast path's B = A A^T, c = A y and B U -- is then an integer
# below 2^52 (checked), so it is exact in any summation order, and so is the update.  A dropped, doubled or misplaced
# contribution of any size shows up as a bit difference against plain fp64 torch on the host.
EXACT_ETA = 2.0 ** -21
EXACT_S2 = 0.25


class ExactProblem:
    def __init__(self, mk, n, j, seed=0, amax=3, umax=3, ymax=8, xmax=3, lam_exp=(-2, 3)):
        g = torch.Generator().manual_seed(seed)

        def ints(shape, m):
            return torch.randint(-m, m + 1, shape, generator=g, dtype=torch.int64).double()

        self.mk, self.n, self.j = mk, n, j
        self.a = ints((mk, n), amax)
        self.u = ints((mk, j), umax)
        self.y = ints((n,), ymax)
        self.xi = self.injected = ints((mk, j), xmax)  # (the orthonormal basis' noise is white: injected as it is)
        self.lam = 2.0 ** torch.randint(lam_exp[0], lam_exp[1] + 1, (mk,), generator=g, dtype=torch.int64).double()
        self.bound = self._bound(amax, umax, ymax, xmax, lam_exp)

    def _bound(self, amax, umax, ymax, xmax, lam_exp):
        """The largest magnitude any route's intermediate can reach (sum of absolute values); asserts it stays below 2^52."""
        mk, n = self.mk, self.n
        nh = n // 2
        f = mk * amax * umax
        g = 4 * (f + ymax)
        plain = n * amax * g
        s = [2 * amax, 3 * amax, 2 * amax, 4 * amax]  # S1..S4
        t = [2 * g, 3 * g, 2 * g, 4 * g]  # T1..T4
        # P1 = A11 G11, P2 = A12 G21, P3 = S4 G22, P4 = A22 T4, P5 = S1 T1, P6 = S2 T2, P7 = S3 T3; D: sums of them
        prods = [nh * l * r for l, r in ((amax, g), (amax, g), (s[3], g), (amax, t[3]), (s[0], t[0]), (s[1], t[1]), (s[2], t[2]))]
        bb = n * amax * amax  # B = A A^T
        fast = mk * bb * umax + n * amax * ymax  # B U - c
        biggest = max(f, g, plain, *prods, sum(prods), bb, 4 * fast)
        assert biggest < 2.0 ** 52, f"exact problem out of range: {biggest:.3e}"
        # the update -eta D - eta U / lam + sqrt(2 eta) xi (+ U) for step sizes eta / 4 .. 4 eta, in units of its finest bit
        step = 4 * EXACT_ETA * (max(plain, sum(prods), 4 * fast) + umax * 2.0 ** -lam_exp[0]) + 2.0 ** -9 * xmax + umax
        unit = EXACT_ETA / 4 * 2.0 ** -lam_exp[1]
        assert step / unit < 2.0 ** 52, "exact problem: the update does not fit one fp64 mantissa"
        return biggest

    def cost(self, P):
        return P.costs.GaussianCost(EXACT_S2, self.y, P.links.IdentityLinkFunction())

    def basis(self, P):
        return P.basis.OrthonormalBasis.from_projection(self.a.cuda(), self.lam.cuda(), poison_padding=True)

    def step(self, cols=None, eta=EXACT_ETA, noise=True, new_state=False):
        """The step on columns ``cols`` (default: all) written out in fp64 (exact here), and the energies of its input
        particles.  ``eta``: a number or one step size per column of ``cols``."""
        cols = torch.arange(self.j) if cols is None else torch.as_tensor(cols)
        uc = self.u[:, cols]
        f = self.a.T @ uc
        d = self.a @ ((f - self.y[:, None]) / EXACT_S2)
        eta = torch.as_tensor(eta, dtype=torch.float64).expand(len(cols))[None, :]
        out = -eta * d - eta * uc / self.lam[:, None]
        if noise:
            out = out + (2 * eta).sqrt() * self.xi[:, cols]
        if new_state:
            out = uc + out
        e = ((f - self.y[:, None]) ** 2).sum(0) / (2 * EXACT_S2) + 0.5 * (uc * uc / self.lam[:, None]).sum(0)
        return out, e


# ---- exact problems of the inducing-point basis -------------------------------------------------------------------------------
# k(Z,Z) = Lc Lc^T with Lc = diag(d) (I + Nl): d powers of two, Nl strictly lower triangular with small integers at (odd row,
# even column) only, so that Nl Nl = 0 and Lc^-1 = (I - Nl) diag(1 / d) exactly.  Every pivot of the factorisation is a power
# of four (sqrt and reciprocal exact), every Schur complement, substitution partial sum, solve, projection, back-projection,
# whitened operator and update a dyadic number of a few dozen bits: exact in any summation order (checked by _bound from the
# data, not assumed), so every route of the basis must reproduce plain fp64 torch on the host bit for bit, and the
# conditioning of k(Z,Z) does not enter.
def _unit(x):
    """the finest bit of a tensor of dyadic numbers: the largest power of two that divides every entry (1 for all zeros)"""
    nz = x[x != 0]
    if nz.numel() == 0:
        return 1.0
    _, e = torch.frexp(nz)  # x = m 2^e, m in [0.5, 1) with 53 bits: the lowest set bit of m 2^53 gives the unit
    mant = (torch.ldexp(nz, 53 - e)).abs().to(torch.int64)
    low = mant & -mant
    return float(torch.ldexp(low.double(), e - 53).min())


class ExactIpbProblem:
    """M inducing points, N data rows, J particles.  ``nmax``: range of Nl's entries, ``emax``: d = 2^e with e in 0..emax,
    ``kmax`` / ``umax`` / ``ximax`` / ``ymax``: ranges of k(Z,X), U, xi, y.  ``eta``: the step size the bound is proved for
    (and for eta / 4 .. 4 eta); ``chain``: number of consecutive whitened steps the bound must also hold for."""

    def __init__(self, m, n, j, seed=0, nmax=2, emax=2, kmax=3, umax=3, ximax=3, ymax=8, eta=EXACT_ETA, chain=0):
        g = torch.Generator().manual_seed(seed)

        def ints(shape, r):
            return torch.randint(-r, r + 1, shape, generator=g, dtype=torch.int64).double()

        self.m, self.mk, self.n, self.j, self.eta, self.seed = m, m, n, j, eta, seed
        idx = torch.arange(m)
        mask = (idx[:, None] % 2 == 1) & (idx[None, :] % 2 == 0) & (idx[:, None] > idx[None, :])
        self.nl = ints((m, m), nmax) * mask
        self.d = 2.0 ** torch.randint(0, emax + 1, (m,), generator=g, dtype=torch.int64).double()
        eye = torch.eye(m, dtype=torch.float64)
        self.lc = self.d[:, None] * (eye + self.nl)
        self.linv = (eye - self.nl) / self.d[None, :]
        self.kzz = self.lc @ self.lc.T
        self.kzx = ints((m, n), kmax)
        self.u = ints((m, j), umax)
        self.xi = ints((m, j), ximax)
        self.y = ints((n,), ymax)
        self.e = self.injected = self.lc @ self.xi  # the coloured noise pls_ipb_step takes as injected noise: integers
        self.s = self.linv @ self.u  # the whitened particles
        self.bits = {}
        self._bound(chain)
        self.energy_exact = max(v for k, v in self.bits.items() if k.startswith("energy")) < 52

    # -- the bit budget -------------------------------------------------------------------------------------------------------
    def _fits(self, name, a, b, limit=52):
        """The product a @ b in any summation order: (sum of absolute values) / (finest bit of a term) must stay below
        2^limit; returns the product, computed in fp64 (then exact)."""
        unit = _unit(a) * _unit(b)
        bits = math.log2(max((a.abs() @ b.abs()).max().item() / unit, 1.0))
        self.bits[name] = max(self.bits.get(name, 0.0), bits)
        assert bits < limit, f"exact inducing-point problem {self.m}x{self.n}x{self.j}: {name} needs {bits:.1f} bits"
        return a @ b

    def _fits_sum(self, name, *terms, limit=52):
        unit = min(_unit(t) for t in terms)
        bits = math.log2(max(sum(t.abs() for t in terms).max().item() / unit, 1.0))
        self.bits[name] = max(self.bits.get(name, 0.0), bits)
        assert bits < limit, f"exact inducing-point problem {self.m}x{self.n}x{self.j}: {name} needs {bits:.1f} bits"

    def _bound(self, chain):
        """Proves from the data that every product a route forms is exact: the factorisation's Schur complements, both
        substitution sweeps, the inverse-factor products, the explicit inverse, the projection, the back-projection, the
        Gaussian constants, the whitened operators and steps, the prior-row operand (M a power of four), the final update
        for step sizes eta / 4 .. 4 eta, and ``chain`` consecutive whitened steps.  The energies' budget is recorded
        (bits["energy ..."]) and decides ``energy_exact``; everything else is asserted."""
        m, f = self.m, self._fits
        lc, li, u, kzx, y = self.lc, self.linv, self.u, self.kzx, self.y[:, None]
        f("Lc Lc^T", lc, lc.T)  # the trailing updates of the factorisation, in any blocking
        f("Lc^-1 Lc", li, lc)  # the panels' triangular solves and the inverse factor's substitution
        s = f("Lc^-1 U", li, u)
        f("forward substitution", li, u.abs() + lc.abs() @ s.abs())  # u_b - sum_k L_bk s_k, then the diagonal block's inverse
        v = f("Lc^-T S", li.T, s)
        f("backward substitution", li.T, s.abs() + lc.T.abs() @ v.abs())
        w = f("W = Lc^-T Lc^-1", li.T, li)
        f("W U", w, u)
        f("Lc xi", lc, self.xi)
        fx = f("F = k(X,Z) V", kzx.T, v)
        gr = (fx - y) / EXACT_S2
        self._fits_sum("G = (F - y) / sigma2", fx / EXACT_S2, y / EXACT_S2)
        dd = f("k(Z,X) G", kzx, gr)
        b = f("B = k(Z,X) k(X,Z)", kzx, kzx.T)
        c = f("c = k(Z,X) y", kzx, y)
        bv = f("B V", b, v)
        self._fits_sum("(B V - c) / sigma2", bv / EXACT_S2, c / EXACT_S2)
        bp = b / EXACT_S2 + m * torch.eye(m, dtype=torch.float64)
        t2 = f("Lc^-1 B'", li, bp)
        q = f("Q = Lc^-1 B' Lc^-T", li, t2.T)
        f("Q (other order)", t2, li.T)
        ct = f("c~", li, c / EXACT_S2)
        pt = f("Pt = Lc^-T Q", li.T, q)
        self.q, self.ct = q, ct
        qs = f("Q S", q, s)
        f("P U", pt.T, u)
        self._fits_sum("Q S - c~", qs, ct)
        f("Lc dS", lc, (qs - ct).abs() + 8 * self.xi.abs())
        root = math.isqrt(m)
        if root * root == m and root & (root - 1) == 0:  # sqrt(M) exact: the prior-row operand k(X,Z) Lc^-T over sqrt(M) Lc^-T
            awa = torch.cat([f("k(X,Z) Lc^-T", kzx.T, li.T), root * li.T])
            fa = f("Awa S", awa, s)
            ga = torch.cat([(fa[: self.n] - y) / EXACT_S2, fa[self.n:]])
            f("Awa^T G", awa.T, ga)
        # the update [U +] -eta D - eta M V + sqrt(2 eta) e over eta / 4 .. 4 eta, in units of its finest bit
        for lo, hi in ((self.eta / 4, 4 * self.eta),):
            self._fits_sum("update", u, hi * dd, hi * m * v, math.sqrt(2 * hi) * self.e, lo * dd, lo * m * v, math.sqrt(2 * lo) * self.e)
            self._fits_sum("whitened update", s, hi * qs, hi * ct, math.sqrt(2 * hi) * self.xi, lo * qs, lo * ct,
                           math.sqrt(2 * lo) * self.xi)
        # energies: the three forms the routes use (data term + prior; fast path from V, B V, c; whitened quadratic form)
        yty = (y * y).sum()
        self._energy_bits("energy general", ((fx - y) ** 2).sum(0) / (2 * EXACT_S2) + 0.5 * m * (v * v).sum(0), _unit(fx) ** 2)
        self._energy_bits("energy fast", ((v * bv).abs().sum(0) + 2 * (v * c).abs().sum(0) + yty) / (2 * EXACT_S2)
                          + 0.5 * m * (v * v).sum(0), _unit(v) * _unit(bv))
        self._energy_bits("energy whitened", 0.5 * (s * qs).abs().sum(0) + (s * ct).abs().sum(0) + yty / (2 * EXACT_S2),
                          0.5 * _unit(s) * _unit(qs))
        state = s
        for k in range(chain):  # consecutive whitened steps with fresh noise: the state's bits grow every step
            xi = self.chain_noise(k)
            qs = f(f"chain step {k}: Q S", q, state)
            new = state - self.eta * (qs - ct) + math.sqrt(2 * self.eta) * xi
            self._fits_sum(f"chain step {k}: update", state, self.eta * qs, self.eta * ct, math.sqrt(2 * self.eta) * xi)
            state = new

    def _energy_bits(self, name, magnitude, unit):
        self.bits[name] = math.log2(max(magnitude.max().item() / unit, 1.0))

    def chain_noise(self, k):
        g = torch.Generator().manual_seed(1000 + k)
        return torch.randint(-3, 4, (self.m, self.j), generator=g, dtype=torch.int64).double()

    # -- the library's objects ------------------------------------------------------------------------------------------------
    def cost(self, P):
        return P.costs.GaussianCost(EXACT_S2, self.y, P.links.IdentityLinkFunction())

    def basis(self, P, host_factor=False, explicit_inverse=False):
        """the device factorisation of k(Z,Z), or (``host_factor``) the constructed factor uploaded (factor_from_host)"""
        return P.basis.InducingPointBasis.from_gram(self.kzz.cuda(), self.kzx.cuda(), cholesky_factor=self.lc if host_factor else None,
                                                    explicit_inverse=explicit_inverse, poison_padding=True)

    # -- the steps, written out in fp64 on the host (exact here) ----------------------------------------------------------------
    def _drift(self, v, reverse=False):
        """(k(Z,X) G + M V, energies) of V = k(Z,Z)^-1 U; ``reverse``: every contraction summed in the opposite order"""
        mm = (lambda a, b: a.flip(1) @ b.flip(0)) if reverse else (lambda a, b: a @ b)
        f = mm(self.kzx.T, v)
        r = f - self.y[:, None]
        d = mm(self.kzx, r / EXACT_S2) + self.m * v
        e = (r * r).sum(0) / (2 * EXACT_S2) + 0.5 * self.m * (v * v).sum(0)
        return d, e

    def solve(self, u, reverse=False):
        mm = (lambda a, b: a.flip(1) @ b.flip(0)) if reverse else (lambda a, b: a @ b)
        return mm(self.linv.T, mm(self.linv, u))

    def step(self, cols=None, eta=None, noise=True, new_state=False, reverse=False):
        """The step of pls_ipb_step on columns ``cols`` (default: all): -eta k(Z,X) G - eta M V + sqrt(2 eta) e, e = Lc xi the
        injected noise (already coloured, as the entry's contract says), and the energies cost + M/2 |V|^2 of the input
        particles.  ``eta``: a number or one step size per column of ``cols``."""
        cols = torch.arange(self.j) if cols is None else torch.as_tensor(cols)
        eta = torch.as_tensor(self.eta if eta is None else eta, dtype=torch.float64).expand(len(cols))[None, :]
        uc = self.u[:, cols]
        d, e = self._drift(self.solve(uc, reverse), reverse)
        out = -eta * d
        if noise:
            out = out + (2 * eta).sqrt() * self.e[:, cols]
        return (uc + out if new_state else out), e

    def whitened_step(self, cols=None, eta=None, noise=True, new_state=False, state=None, xi=None, reverse=False):
        """The same step in whitened coordinates S = Lc^-1 U (default state: the whitened particles): dS = Lc^-1 (-eta k(Z,X) G
        - eta M V) + sqrt(2 eta) xi with V = Lc^-T S; the injected noise xi is white (pls_ipb_whitened_step's contract)."""
        mm = (lambda a, b: a.flip(1) @ b.flip(0)) if reverse else (lambda a, b: a @ b)
        cols = torch.arange(self.j) if cols is None else torch.as_tensor(cols)
        eta = torch.as_tensor(self.eta if eta is None else eta, dtype=torch.float64).expand(len(cols))[None, :]
        sc = (self.s if state is None else state)[:, cols]
        d, e = self._drift(mm(self.linv.T, sc), reverse)
        out = -eta * mm(self.linv, d)
        if noise:
            out = out + (2 * eta).sqrt() * (self.xi if xi is None else xi)[:, cols]
        return (sc + out if new_state else out), e


# the shapes tests/test_gpu_exact_ipb.py runs; tests/test_host_logic.py proves on the CPU that the reference alone is exact on each
IPB_FACTOR_M = [1, 2, 17, 63, 64, 65, 127, 128, 129, 200, 257, 520, 1024, 1153]  # chol.hip: panel 64, block 128, strip depth 32
# (M, J): J in {1, 5, 64, 65, 700, 1024, 4100} across M; 960 and 1088 have an odd number of 64-row tile rows (ragged pairs)
IPB_SOLVE_CASES = [(1, 1), (2, 5), (17, 64), (63, 65), (64, 5), (65, 700), (127, 64), (128, 65), (129, 1024), (200, 5), (257, 700),
                   (520, 65), (960, 1024), (1088, 700), (1024, 1024), (1024, 700), (1024, 4100), (1153, 64)]
# (M, N, J): N off the 128 grid, ragged last column tiles, the narrow shard M = 1024 with J = 700 / 1024, the mid-size config
IPB_STEP_SHAPES = [(64, 300, 40), (200, 1500, 333), (129, 5000, 200), (1024, 3000, 700), (1024, 3000, 1024), (1024, 8000, 512)]
# (M, N, J, rows per chunk): N = 300 runs in one split-K slab, N = 20000 in several; the last: three chunks
IPB_GENERAL_CASES = [(200, 300, 333, None), (200, 20000, 333, None), (200, 20000, 333, 20000 // 3), (1024, 8000, 512, None)]
IPB_ONE_LAUNCH_SHAPES = [(100, 10, 64), (333, 17, 37), (1000, 32, 100), (1100, 128, 90), (520, 65, 16)]  # (N, M, J)
IPB_PREP_M = [1, 2, 3, 5, 15, 16, 17, 18, 31, 32, 33, 48, 49, 63, 64, 65, 80, 81, 97, 112, 113, 127]
IPB_WHITENED_GENERIC_SHAPES = [(50, 1, 8), (100, 4, 64), (333, 16, 37), (1000, 64, 100)]  # (N, M, J), M a power of four
# three consecutive whitened steps: every step multiplies the state's bits by those of eta Q, so the ranges shrink (Nl, k(Z,X) in
# [-1, 1], d = 1) and eta grows until the third step's Q S fits one mantissa (ExactIpbProblem._bound, chain=3)
IPB_CHAIN_CASES = [(200, 100, 70, dict(eta=2.0 ** -13, nmax=1, emax=0, kmax=1)),
                   (320, 100, 130, dict(eta=2.0 ** -15, nmax=1, emax=0, kmax=1, umax=1, ymax=2)),
                   (64, 60, 40, dict(eta=2.0 ** -11, nmax=1, emax=0, kmax=1))]
_exact_ipb = {}


def exact_ipb(m, n, j, **kw):
    """the exact problem of a shape, built (and its bit budget proved) once per process"""
    key = (m, n, j, tuple(sorted(kw.items())))
    if key not in _exact_ipb:
        if len(_exact_ipb) >= 6:
            _exact_ipb.clear()
        _exact_ipb[key] = ExactIpbProblem(m, n, j, seed=m + n + j, **kw)
    return _exact_ipb[key]


def exact_ipb_cases():
    """every (M, N, J, options) tests/test_gpu_exact_ipb.py builds"""
    cases = [(m, 16, 8, {}) for m in IPB_FACTOR_M] + [(m, 16, j, {}) for m, j in IPB_SOLVE_CASES] + [(200, 16, 65, {})]
    cases += [(m, n, j, {}) for m, n, j in IPB_STEP_SHAPES] + [(m, n, j, {}) for m, n, j, _ in IPB_GENERAL_CASES]
    cases += [(m, n, j, {}) for n, m, j in IPB_ONE_LAUNCH_SHAPES + IPB_WHITENED_GENERIC_SHAPES]
    cases += [(m, 200 + m, j, {}) for m in IPB_PREP_M for j in (1, 17, 50)]
    cases += [(m, n, j, dict(chain=3, **kw)) for m, n, j, kw in IPB_CHAIN_CASES]
    return list({(m, n, j, tuple(sorted(kw.items()))): (m, n, j, kw) for m, n, j, kw in cases}.values())


# ---- the checks both exact files share (tests/test_gpu_exact_step.py, tests/test_gpu_exact_ipb.py) ----------------------------
BLOCK_ETAS = [EXACT_ETA, 0.0, 4 * EXACT_ETA, EXACT_ETA / 4]  # sqrt(2 eta) = 2^-10, 0, 2^-9, 2^-11: all exact


class option:
    def __init__(self, P, opt, mode):
        self.L, self.lib, self.opt, self.mode = P.pkg._lib, P.pkg._lib.load(), opt, mode

    def __enter__(self):
        self.prev = self.lib.pls_get_option(self.opt)
        self.L.check(self.lib.pls_set_option(self.opt, self.mode), "pls_set_option")

    def __exit__(self, *exc):
        self.L.check(self.lib.pls_set_option(self.opt, self.prev), "pls_set_option")
        return False


def assert_exact(ex, got, cols=None, energy=None, eta=EXACT_ETA, noise=True, new_state=False, what=""):
    want, e_want = ex.step(cols, eta, noise, new_state)
    got = got.cpu() if cols is None else got.cpu()[:, cols]
    assert torch.isfinite(got).all(), what
    bad = (got != want).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows differ from the exact step, first {bad[:8].tolist()}, " \
                             f"max |diff| {(got - want).abs().max().item():.3e}"
    if energy is not None:
        e = energy.cpu() if cols is None else energy.cpu()[cols]
        rel = ((e - e_want).abs() / e_want.abs()).max().item()
        assert rel <= 1e-13, f"{what}: energy by-product, relative error {rel:.2e}"
        if getattr(ex, "energy_exact", False):  # (the quadratic forms fit one mantissa too: ExactIpbProblem._bound)
            assert torch.equal(e, e_want), f"{what}: energy by-product differs from the exact one, relative error {rel:.2e}"


def run_forms(P, ex, gb, cost, cols, what, force_generic=True):
    """The step out of place (fresh output, with energies), into a strided output buffer (guard columns untouched), as the
    new state, and with per-block step sizes (one block frozen) -- each against the exact step."""
    j = ex.j
    u = ex.u.cuda()
    xi = P.basis.NoiseSpec(injected=ex.injected.cuda())
    e = torch.full((j,), float("nan"), device="cuda")
    got = gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, input_energy=e)
    assert_exact(ex, got, cols, energy=e, what=f"{what}: out of place")
    wide = torch.full((ex.mk, j + 64), float("nan"), device="cuda")
    out = wide[:, :j]
    gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, out=out)
    assert_exact(ex, out, cols, what=f"{what}: strided output")
    assert wide[:, j:].isnan().all(), f"{what}: the step wrote past J"
    new = gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, new_state=True)
    assert_exact(ex, new, cols, new_state=True, what=f"{what}: new state")
    bc = -(-j // len(BLOCK_ETAS))
    blocks = P.basis.BlockSpec(bc, torch.tensor(BLOCK_ETAS, device="cuda"))
    got = gb.fused_step(cost, u, 0.0, noise=xi, force_generic=force_generic, blocks=blocks, new_state=True)
    etas = torch.tensor(BLOCK_ETAS)[torch.arange(j) // bc]
    assert_exact(ex, got, cols, eta=etas if cols is None else etas[cols], new_state=True, what=f"{what}: blocks")
    assert torch.equal(got[:, bc:2 * bc].cpu(), ex.u[:, bc:2 * bc]), f"{what}: a frozen block moved"
    with pytest.raises(P.pkg._lib.PlsHipError):  # in place: the entries refuse an output that aliases the particles
        P.pkg._lib.check(gb._route(cost, j, force_generic).call(None, u.data_ptr(), j, j, EXACT_ETA, xi.desc(), u.data_ptr(), j,
                                                                 0, None, None, 0, P.pkg._lib.stream_ptr()), "in place")


def spread_columns(j, per_tile=2, seed=0):
    """A sorted column sample that holds both ends of every 128-column tile of J's first half, ``per_tile`` columns in
    between, and each one's Winograd partner c + J/2."""
    g = torch.Generator().manual_seed(seed)
    jh = j // 2
    cols = set()
    for t0 in range(0, jh, 128):
        w = min(128, jh - t0)
        cols.update((t0, t0 + w - 1))
        cols.update((t0 + torch.randint(0, w, (per_tile,), generator=g)).tolist())
    first = sorted(cols)
    return torch.tensor(first + [c + jh for c in first])


# ---- the Winograd route of the general step: probes and workspaces --------------------------------------------------------
def wino_planes_bytes(mk, n):
    """The four left-hand planes S1..S4 (csrc/step_plan.h wino_left_plane_bytes) of a basis, whether or not it takes the route."""
    return 4 * (-(-(n // 2) * (mk // 2) * 8 // 256) * 256)


def wino_one_chunk_bytes(mk, n, j):
    """A workspace that holds the Winograd route's layout for all N/2 paired rows at any slab count (<= 16)."""
    mh, nh, jh = mk // 2, n // 2, j // 2

    def up(x):
        return -(-x // 256) * 256

    return 7 * 16 * up(mh * jh * 8) + up(max(32, -(-nh // 32)) * j * 8) + 7 * up(nh * jh * 8)


def step_wg(P, gb, cost, u, eta, planes, noise=None, blocks=None, out=None, new_state=False, energy=None, ws_bytes=None):
    """One general step (force_generic) straight through pls_onb_step_wg / pls_onb_step_blocks_wg with the left-hand planes
    ``planes``; ``ws_bytes``: the workspace (default: what fused_step would hand in)."""
    L = P.pkg._lib
    lib = L.load()
    j = u.shape[1]
    if ws_bytes is None:
        ws_bytes = gb.step_workspace_bytes(cost, j, energy is not None, force_generic=True)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device="cuda")
    if out is None:
        out = torch.empty(u.shape, dtype=torch.float64, device="cuda")
    nd = (noise if noise is not None else P.basis.NoiseSpec(none=True)).desc()
    mode = L.OUT_NEW_STATE if new_state else L.OUT_DELTA
    head = (gb._desc(), cost.desc(), cost.y_device().data_ptr(), u.data_ptr(), L.ld(u), j)
    tail = (nd, out.data_ptr(), L.ld(out), mode, 1, planes.data_ptr(), planes.numel() * 8, L.ptr(energy), ws.data_ptr(), ws_bytes,
            L.stream_ptr())
    if blocks is None:
        L.check(lib.pls_onb_step_wg(*head, float(eta), *tail), "pls_onb_step_wg")
    else:
        L.check(lib.pls_onb_step_blocks_wg(*head, blocks.desc(), *tail), "pls_onb_step_blocks_wg")
    return out


def nan_planes(mk, n):
    return torch.full((wino_planes_bytes(mk, n) // 8,), float("nan"), dtype=torch.float64, device="cuda")


class winograd_option:
    """with winograd_option(P, 0 | 1): PLS_OPT_WINOGRAD for the block, restored after"""

    def __init__(self, P, mode):
        self.L, self.lib, self.mode = P.pkg._lib, P.pkg._lib.load(), mode

    def __enter__(self):
        self.prev = self.lib.pls_get_option(self.L.OPT_WINOGRAD)
        self.L.check(self.lib.pls_set_option(self.L.OPT_WINOGRAD, self.mode), "pls_set_option")

    def __exit__(self, *exc):
        self.L.check(self.lib.pls_set_option(self.L.OPT_WINOGRAD, self.prev), "pls_set_option")
        return False


def probe_winograd(P, gb, cost, u, eta=EXACT_ETA, **kw):
    """Route probe that does not depend on rounding: the step with left-hand planes of NaN.  Returns True when the Winograd
    route ran -- then exactly the three quadrants whose products read S1..S4 are NaN (D11 = A11 G11 + A12 G21 reads none) --
    and False when it did not, in which case the output equals the plain route's bit for bit.  Anything else fails."""
    mk, j = gb.approximation_dimension, u.shape[1]
    out = step_wg(P, gb, cost, u, eta, nan_planes(mk, gb._n), **kw)
    fin = torch.isfinite(out)
    if not fin.all():
        mh, jh = mk // 2, j // 2
        assert fin[:mh, :jh].all(), "the Winograd route's top-left quadrant read the left-hand planes"
        assert not fin[mh:].any() and not fin[:mh, jh:].any(), "a quadrant of the Winograd route did not read its products"
        return True
    with winograd_option(P, 0):
        plain = step_wg(P, gb, cost, u, eta, nan_planes(mk, gb._n), **kw)
    assert torch.equal(out, plain), "outside the Winograd route the step differs from the plain route's"
    return False


# (M_k, N, J) of the Winograd route's envelope (tests/test_gpu_winograd.py); tests/test_winograd_host.py checks their plans.
# In wino_one_chunk_bytes each takes one chunk of all paired rows: M_k = 528 (M_k / 2 = 264: edge tiles in the products and
# the update), J = 2176 (J / 2 = 1088: a 64-column J edge tile), N = 16388 (N / 2 = 8194: a paired-row edge), the route's
# minimum sizes, and a shape whose products run in one split-K slab (the others: several).
WINO_EDGES = [(528, 16384, 2048), (512, 16384, 2176), (512, 16388, 2048), (512, 16384, 2048), (512, 16384, 18688)]
# 7 x 2 x 73 = 1022 product tiles: two rounds of 512 workgroups without split-K (csrc/step_plan.h wino_split_k)
WINO_ONE_SLAB = (512, 16384, 18688)
# in 9/10 of the plain route's all-rows workspace: three chunks (9216 + 9216 + 1568 paired rows)
WINO_THREE_CHUNKS = (512, 40000, 2048)
# just outside the route: M_k, N, J below a limit or off its grid
WINO_OUTSIDE = [(496, 16384, 2048), (512, 16380, 2048), (512, 16384, 1920), (512, 16384, 2112)]


# ---- selector problems: G observable bit for bit through a step, for any cost ---------------------------------------------------
# One carrier direction k0 has A[k0, n] = c_n (signed powers of two, 2^-3 .. 2^3) and U[k0, j] = V_j (any nonzero double); every
# other row of U is zero.  So F[n, j] = c_n V_j exactly in any summation order (one product by a power of two plus zeros): F
# is arbitrary, finite and nonzero, and runs through the regimes of the pair's truth module.  Every other direction k carries one
# probe entry A[k, n_k] = 2^p_k and zeros, so D[k, j] = 2^p_k G[n_k, j] exactly, the prior term U[k, j] / lambda_k is zero,
# and without noise (or with injected zeros) out[k, j] = -eta 2^p_k G[n_k, j] with eta a power of two: not one rounding after
# cost_deriv.  A probe row of a step therefore shows G[n_k, :] bit for bit, on any route, in any tile position.
SELECTOR_PLACEMENTS = ["head", "half", "tail", "spread"]


def selector_values(pair, pset="a"):
    """the finite f of the pair's truth grid with |f| >= 1e-30 and inside the family's SELECTOR_RANGE: the regimes the
    carrier values run through; and the grid's labels"""
    y, f, _ = truth_module(pair).grid(pair, pset)
    a = np.abs(f)
    keep = np.isfinite(f) & (a >= 1e-30) & truth_module(pair).SELECTOR_RANGE[pair](a)
    return np.unique(f[keep]), y


class SelectorProblem:
    """M_k directions, N data rows, J particles for the (cost, link) pair ``pair``.  ``placement``: where the probe rows n_k
    sit -- "head": rows 0, 1, ... (every row slot of the first tiles), "half": from N / 2 (the second operand of paired
    tiles), "tail": the last rows (the ragged last tile), "spread": a seeded sample that holds row 0 and row N - 1."""

    def __init__(self, pair, mk, n, j, placement="head", seed=0, pset="a", k0=None):
        g = torch.Generator().manual_seed(seed)
        self.pair, self.pset, self.mk, self.n, self.j, self.placement = pair, pset, mk, n, j, placement
        self.k0 = k0 = (mk // 3 if k0 is None else k0)
        vals, ys = selector_values(pair, pset)

        def carrier_values(g):
            """V_j: the grid's values (every regime), each also scaled by a full-mantissa factor near one, and plain normals"""
            pick = torch.as_tensor(vals)[torch.randint(0, len(vals), (j,), generator=g)]
            jiggle = 1 + (torch.rand(j, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -3
            third = torch.arange(j) % 3
            v = torch.where(third == 0, pick, torch.where(third == 1, pick * jiggle, 1.5 * torch.randn(j, generator=g, dtype=torch.float64)))
            v[v == 0] = 0.75
            return v

        def labels(g):
            return torch.as_tensor(ys)[torch.randint(0, len(ys), (n,), generator=g)]

        self.v = carrier_values(g)
        self.c = (2.0 ** torch.randint(-3, 4, (n,), generator=g).double()) * (1 - 2 * torch.randint(0, 2, (n,), generator=g).double())
        self.c[torch.arange(n) % 3 == 0] = 1.0  # a third of the rows see the carrier values themselves
        self.y = labels(g)
        self.lam = 2.0 ** torch.randint(-2, 4, (mk,), generator=g, dtype=torch.int64).double()
        if truth_module(pair).OWN_CARRIER_STREAM:
            # the family's carrier values and labels come from a generator of their own; the draws above still advance the
            # problem's generator, so that everything else of the construction is what it is for any other family
            own = torch.Generator().manual_seed(seed + 4242)
            self.v = carrier_values(own)
            self.y = labels(own)
        others = [k for k in range(mk) if k != k0]
        nprobe = min(len(others), n)
        if placement == "head":
            rows = torch.arange(nprobe)
        elif placement == "half":
            rows = (n // 2 + torch.arange(nprobe)) % n
        elif placement == "tail":
            rows = n - 1 - torch.arange(nprobe)
        else:
            perm = torch.randperm(n, generator=g)[:nprobe]
            perm = perm[(perm != 0) & (perm != n - 1)]
            rows = torch.cat([torch.tensor([0, n - 1]), perm])[:nprobe] if n > 1 else perm
            rows = torch.unique(rows)
        nprobe = len(rows)
        order = torch.randperm(len(others), generator=g)[:nprobe]
        self.probe_k = torch.as_tensor(others)[order]  # direction k of probe i
        self.probe_n = rows[torch.randperm(nprobe, generator=g)]  # its data row n_k
        self.probe_p = torch.randint(-2, 3, (nprobe,), generator=g)  # A[k, n_k] = 2^p
        self.a = torch.zeros(mk, n, dtype=torch.float64)
        self.a[k0] = self.c
        self.a[self.probe_k, self.probe_n] = 2.0 ** self.probe_p.double()
        self.u = torch.zeros(mk, j, dtype=torch.float64)
        self.u[k0] = self.v
        self.injected = torch.zeros(mk, j, dtype=torch.float64)
        self._check()

    def _check(self):
        """From the data: F = A^T U equals c_n V_j in either summation order, is finite and nonzero, no product left the
        normal range (so it is exact), and every probe direction holds exactly one entry, a power of two."""
        cols = torch.unique(torch.linspace(0, self.j - 1, min(self.j, 192)).long())  # (a column sample keeps wide J cheap)
        f, u = self.f(cols), self.u[:, cols]
        assert torch.equal(self.a.T @ u, f) and torch.equal(self.a.T.flip(1) @ u.flip(0), f)
        f = self.f()
        assert torch.isfinite(f).all() and (f.abs() >= 2.0 ** -1000).all() and (f.abs() <= 2.0 ** 1000).all()
        m, _ = torch.frexp(self.c)
        assert (m.abs() == 0.5).all() and (self.c.abs() >= 2.0 ** -3).all() and (self.c.abs() <= 8).all()
        rest = self.a.clone()
        rest[self.k0] = 0
        assert ((rest != 0).sum(1)[self.probe_k] == 1).all() and (rest != 0).sum() == len(self.probe_k)
        assert len(torch.unique(self.probe_n)) == len(self.probe_n) == len(torch.unique(self.probe_k))
        assert (self.u[torch.arange(self.mk) != self.k0] == 0).all() and (self.v != 0).all()
        ml, _ = torch.frexp(self.lam)
        assert (ml == 0.5).all()
        self.state = self.u  # what a new-state step adds its update to
        self.row_scale = torch.ones(self.mk, dtype=torch.float64)

    def prior_row(self, cols):
        """the prior term of the carrier row, per unit eta"""
        return self.v[cols] / self.lam[self.k0]

    def prior_energy(self, col):
        return float(self.v[col]) ** 2 / (2 * float(self.lam[self.k0]))

    def f(self, cols=None):
        v = self.v if cols is None else self.v[torch.as_tensor(cols)]
        return self.c[:, None] * v[None, :]

    def cost(self, P, force_autograd=False):
        cost = truth_module(self.pair).gpu_cost(P, self.pair, self.pset, self.y)
        if force_autograd:  # the step takes the derivative mode from the cost's descriptor
            plain = cost.desc
            cost.desc = lambda force_autograd=False: plain(force_autograd=True)
        return cost

    def basis(self, P):
        return P.basis.OrthonormalBasis.from_projection(self.a.cuda(), self.lam.cuda(), poison_padding=True)

    def g_direct(self, P, cost, cols=None, force_autograd=False):
        """G on the host-built F through the element-wise entry (tests/test_gpu_cost_elements.py holds it to the truth)"""
        return cost.calculate_cost_derivative(self.f(cols).cuda(), force_autograd=force_autograd).cpu()

    def g_gauss_fma(self, g, cols=None, rows=None):
        """Gaussian/identity on the routes whose forward GEMM carries the cost in its epilogue: G = fma(F, 1 / sigma2,
        -(1 / sigma2) y) (csrc/cost_epilogues.h EpiGaussDeriv: one fma per element in every tile shape), not the element-wise
        entry's (F - y) (1 / sigma2).  That operation order, emulated exactly (rational arithmetic, one rounding), replaces
        ``g`` on ``rows`` (default: the probe rows); returns (G, carrier slack): the other rows keep the element-wise G, and
        the carrier row may differ by the two formulas' roundings, sum_n |c_n| 2^-52 (|F| + |y|) / sigma2 per unit eta."""
        from fractions import Fraction

        assert self.pair == "gaussian/identity"
        ip0 = 1.0 / truth_module(self.pair).PARAMS[self.pset]["gaussian"][0]
        f = self.f(cols)
        rows = self.probe_n if rows is None else rows
        g = g.clone()
        fi = Fraction(ip0)
        for a in torch.as_tensor(rows).tolist():
            c = Fraction(-ip0 * float(self.y[a]))
            g[a] = torch.tensor([float(Fraction(v) * fi + c) for v in f[a].tolist()], dtype=torch.float64)
        slack = (self.c.abs()[:, None] * 2.0 ** -52 * (f.abs() + self.y.abs()[:, None]) * ip0).sum(0)
        return g, slack

    def values_direct(self, P, cols=None):
        """cost(y_n, F[n, j]) per element through the element-wise entry pls_cost_value (which sums over rows: the rows of one
        label go in as a single row, every element a column of its own; tests/test_gpu_cost_elements.py holds the entry to
        the truth)"""
        f = self.f(cols)
        out = torch.empty_like(f)
        for yy in torch.unique(self.y).tolist():
            rows = (self.y == yy).nonzero().flatten()
            cost = truth_module(self.pair).gpu_cost(P, self.pair, self.pset, torch.tensor([yy], dtype=torch.float64))
            out[rows] = cost.calculate_cost(f[rows].reshape(1, -1).cuda()).cpu().reshape(len(rows), -1)
        return out

    def energy_direct(self, P, cols=None, gauss_fma=False):
        """(want, tolerance) of the energies on ``cols``: fsum of values_direct plus the prior, within the N roundings of any
        summation order (cost_value is evaluated without contraction, so every route forms the same element values).
        ``gauss_fma``: the Gaussian/identity GEMM epilogues form the value as G^2 sigma2 / 2 from G = fma(F, 1 / sigma2,
        -(1 / sigma2) y), which differs from (F - y)^2 / (2 sigma2) by 2^-52 |F - y| (|F| + |y|) / sigma2 per element."""
        cols = torch.arange(self.j) if cols is None else torch.as_tensor(cols)
        v = self.values_direct(P, cols)
        assert torch.isfinite(v).all()
        prior = torch.tensor([self.prior_energy(c) for c in cols.tolist()], dtype=torch.float64)
        want = torch.tensor([math.fsum(v[:, b].tolist()) for b in range(len(cols))], dtype=torch.float64) + prior
        tol = (self.n + 2) * 2.0 ** -53 * (v.abs().sum(0) + prior) + 2.0 ** -52 * want.abs()
        if gauss_fma:
            f = self.f(cols)
            s2 = truth_module(self.pair).PARAMS[self.pset]["gaussian"][0]
            tol = tol + 2.0 ** -51 * ((f - self.y[:, None]).abs() * (f.abs() + self.y.abs()[:, None])).sum(0) / s2
        return want, tol

    def expected(self, g, cols=None, eta=EXACT_ETA, new_state=False):
        """(want, probe mask, carrier tolerance) of the step on columns ``cols`` given G = g_direct there.  ``want``: exact on
        every row but k0 (probe rows -eta 2^p G[n_k], the others 0); row k0 holds fsum_n c_n G[n, j] and the prior, and may
        differ by N 2^-53 sum_n |c_n G[n, j]| + 2 ulp.  Checks that no probe value over- or underflows after scaling."""
        cols = torch.arange(self.j) if cols is None else torch.as_tensor(cols)
        eta = torch.as_tensor(eta, dtype=torch.float64).expand(len(cols))[None, :]
        m, _ = torch.frexp(eta[eta != 0])
        assert (m == 0.5).all(), "the step sizes must be powers of two"
        assert torch.isfinite(g).all(), "the selector problem's G must be finite (choose the carrier values accordingly)"
        gp = g[self.probe_n] * (2.0 ** self.probe_p.double() * self.row_scale[self.probe_k])[:, None]
        scaled = -eta * gp
        live = (gp != 0) & (eta != 0)
        assert (scaled[live].abs() >= 2.0 ** -1000).all() and (scaled.abs() <= 2.0 ** 1000).all(), "a probe value leaves the range"
        want = torch.zeros(self.mk, len(cols), dtype=torch.float64)
        want[self.probe_k] = scaled
        terms = self.c[:, None] * g  # exact: powers of two
        carrier = torch.tensor([math.fsum(terms[:, b].tolist()) for b in range(len(cols))], dtype=torch.float64)
        prior = self.prior_row(cols)
        rs = self.row_scale[self.k0]  # (a power of two)
        want[self.k0] = (-eta[0] * carrier - eta[0] * prior) * rs
        mag = terms.abs().sum(0)
        tol = rs * eta[0].abs() * (self.n * 2.0 ** -53 * mag + 2.0 ** -51 * (carrier.abs() + prior.abs()) + getattr(self, "carrier_slack", 0.0))
        if new_state:
            want[self.k0] = want[self.k0] + self.state[self.k0, cols]
            tol = tol + 2.0 ** -52 * want[self.k0].abs()
        probe = torch.ones(self.mk, dtype=torch.bool)
        probe[self.k0] = False
        return want, probe, tol

    def energy_truth(self, cols):
        """per column: the sum of the mpmath cost values plus the exact prior V_j^2 / (2 lambda_k0), sum_n |cost_n|, and
        the sum of the elements' error units (the larger of an ulp of the value and the truth module's cancel unit; where
        that is a tuple -- the count family's also carries a unit for a subnormal link value -- its first member)"""
        import mpmath as mp

        point_truth = truth_module(self.pair).point_truth
        f = self.f(cols)
        want, mag, units = [], [], []
        for b, col in enumerate(torch.as_tensor(cols).tolist()):
            tot, ab, un = mp.mpf(0), mp.mpf(0), mp.mpf(0)
            for a in range(self.n):
                t, cu = point_truth(self.pair, self.pset, "value", float(self.y[a]), float(f[a, b]))
                cu = cu[0] if isinstance(cu, tuple) else cu
                tot, ab, un = tot + t, ab + abs(t), un + max(cu, abs(t) * mp.mpf(2) ** -52)
            want.append(float(tot + mp.mpf(self.prior_energy(col))))
            mag.append(float(ab))
            units.append(float(un))
        return tuple(torch.tensor(x, dtype=torch.float64) for x in (want, mag, units))


def assert_selector(ex, got, g, cols=None, eta=EXACT_ETA, new_state=False, what=""):
    """probe rows (all rows but the carrier's) bit for bit, the carrier row within its summation bound"""
    want, probe, tol = ex.expected(g, cols, eta, new_state)
    got = got.cpu() if cols is None else got.cpu()[:, torch.as_tensor(cols)]
    bad = (got[probe] != want[probe]).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} probe rows differ from -eta 2^p G[n_k], first (row index among the " \
                             f"non-carrier rows) {bad[:8].tolist()}, max |diff| {(got[probe] - want[probe]).abs().max().item():.3e}"
    err = (got[ex.k0] - want[ex.k0]).abs()
    over = (err > tol).nonzero().flatten()
    assert over.numel() == 0, f"{what}: carrier row over its bound at columns {over[:8].tolist()}: {(err / tol).max().item():.2f} x"


def run_selector_forms(P, ex, gb, cost, g, cols, what, force_generic=True, whitened=False):
    """The step out of place (with and without the energy request: bit-identical), into a strided buffer (guard columns
    untouched), as the new state, and with per-block step sizes -- the probe rows of each against G.  ``whitened``: through
    whitened_step on the whitened particles (SelectorIpbProblem.whitened()).  Returns the energies."""
    j = ex.j
    u = ex.state.cuda()
    xi = P.basis.NoiseSpec(injected=ex.injected.cuda())
    entry = gb.whitened_step if whitened else gb.fused_step
    e = torch.full((j,), float("nan"), device="cuda")
    got = entry(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, input_energy=e)
    assert_selector(ex, got, g, cols, what=f"{what}: out of place")
    bare = entry(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic)
    assert torch.equal(got, bare), f"{what}: asking for the energies moved the step"
    wide = torch.full((ex.mk, j + 64), float("nan"), device="cuda")
    out = wide[:, :j]
    entry(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, out=out)
    assert torch.equal(out, got), f"{what}: strided output"
    assert wide[:, j:].isnan().all(), f"{what}: the step wrote past J"
    new = entry(cost, u, EXACT_ETA, noise=xi, force_generic=force_generic, new_state=True)
    assert_selector(ex, new, g, cols, new_state=True, what=f"{what}: new state")
    bc = -(-j // len(BLOCK_ETAS))
    blocks = P.basis.BlockSpec(bc, torch.tensor(BLOCK_ETAS, device="cuda"))
    got = entry(cost, u, 0.0, noise=xi, force_generic=force_generic, blocks=blocks, new_state=True)
    etas = torch.tensor(BLOCK_ETAS)[torch.arange(j) // bc]
    assert_selector(ex, got, g, cols, eta=etas if cols is None else etas[torch.as_tensor(cols)], new_state=True, what=f"{what}: blocks")
    assert torch.equal(got[:, bc:2 * bc].cpu(), ex.state[:, bc:2 * bc]), f"{what}: a frozen block moved"
    if hasattr(gb, "zero_step_sync"):
        gb.zero_step_sync()
    return e


class SelectorIpbProblem(SelectorProblem):
    """The inducing-point form: k(Z,Z) = diag(4^e_k), so the factor Lc = diag(2^e_k), its inverse and both solves are exact,
    and k(Z,X) built like A above.  The carrier's particles are U[k0] = 4^e V_j, so V = k(Z,Z)^-1 U holds V_j on row k0 and
    zeros elsewhere: F = k(X,Z) V = c_n V_j, and the prior M V vanishes on the probe rows.  ``whitened()`` switches the
    expectations to whitened coordinates S = Lc^-1 U, where a probe row shows -eta 2^p G[n_k] / 2^e_k."""

    def __init__(self, pair, m, n, j, placement="head", seed=0, pset="a"):
        super().__init__(pair, m, n, j, placement, seed, pset)
        g = torch.Generator().manual_seed(seed + 77)
        self.m = m
        self.d = 2.0 ** torch.randint(0, 3, (m,), generator=g, dtype=torch.int64).double()
        self.kzz = torch.diag(self.d * self.d)
        self.kzx = self.a
        self.u = self.u * (self.d * self.d)[:, None]  # exact: powers of four
        self.s = self.u / self.d[:, None]
        assert torch.equal(self.u / (self.d * self.d)[:, None], torch.where(torch.arange(m)[:, None] == self.k0, self.v[None, :], 0.0))
        self.state = self.u

    def whitened(self, on=True):
        self.state = self.s if on else self.u
        self.row_scale = 1.0 / self.d if on else torch.ones(self.m, dtype=torch.float64)
        return self

    def prior_row(self, cols):
        return self.m * self.v[cols]

    def prior_energy(self, col):
        return 0.5 * self.m * float(self.v[col]) ** 2

    def basis(self, P, explicit_inverse=False):
        return P.basis.InducingPointBasis.from_gram(self.kzz.cuda(), self.kzx.cuda(), explicit_inverse=explicit_inverse, poison_padding=True)
