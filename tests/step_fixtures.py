"""Loader for tests/golden/oracle_step_vectors.npz (written by tests/golden/make_oracle_step_vectors.py): the frozen
Langevin step.  Builds the oracle's objects -- and, for the GPU tests, the library's -- from the stored inputs."""
import os

import numpy as np
import torch

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
        self.xi = ints((mk, j), xmax)
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
