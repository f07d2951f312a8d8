"""Solves with k(Z,Z) on real RBF Gram matrices: the cases of tests/test_gpu_solve_accuracy.py, their right-hand sides, the
per-column error measures and the host references.  tests/golden/make_solve_truth.py writes the 50-digit solutions of the
cases with M <= 300 to tests/golden/solve_truth.npz; M = 1024 gets its truth at test time by iterative refinement."""
import hashlib
import os

import numpy as np
import torch

from oracle import pls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
TRUTH = os.path.join(HERE, "golden", "solve_truth.npz")
OUTPUTSCALE = 1.3
COLUMNS = 8
KINDS = ["random"] * 3 + ["smooth"] * 3 + ["rough"] * 2  # right-hand side of each column

# name: (M, D, seed, lengthscale factor, jitter).  The lengthscales are graded, factor * (0.5 .. 1.5) over the dimensions; the
# factor was searched (bisection on torch.linalg.cond, not committed) so that cond(k(Z,Z)) lands near 1e4, 1e8 and 1e12.  The
# last bucket carries the 1e-8 the jitter schedule adds when a pivot fails (then cond(K + 1e-8 I) is what the solves see).
CASES = {}


def _case(name, m, d, seed, factor, jitter=0.0):
    CASES[name] = (m, d, seed, factor, jitter)


for _m, _d, _seed, _factors in ((64, 3, 1, (0.406, 1.11, 2.39)), (128, 3, 2, (0.382, 0.853, 1.57)), (300, 4, 3, (0.474, 0.964, 1.76)),
                               (1024, 8, 4, (0.955, 2.08, 4.67))):
    _case(f"m{_m}/cond1e4", _m, _d, _seed, _factors[0])
    _case(f"m{_m}/cond1e8", _m, _d, _seed, _factors[1])
    _case(f"m{_m}/cond1e12j", _m, _d, _seed, _factors[2], 1e-8)
STORED = [n for n, c in CASES.items() if c[0] <= 300]  # truth in tests/golden/solve_truth.npz
REFINED = [n for n, c in CASES.items() if c[0] > 300]  # truth by iterative refinement at test time


# The truth file holds solutions, not matrices: every machine must regenerate k(Z,Z) and U to the bit.  torch.exp, torch.sin,
# randn and BLAS products take different code paths on different CPUs, so everything here is built from integer draws and
# correctly rounded elementwise operations (+, -, *, /, rint, ldexp: the same result on every IEEE machine), summed in a
# fixed order.
_LN2_HI, _LN2_LO = 0.693147180369123816490, 1.90821492927058770002e-10  # ln 2 = hi + lo, hi with 21 trailing zero bits


def exp_reproducible(x):
    """exp for x <= 0 (numpy float64) to a few ulp (7e-16 relative): x = n ln 2 + r, |r| <= ln 2 / 2, a degree-14 Taylor polynomial in r / 4
    by Horner (separate multiplications and additions), squared twice, scaled by 2^n"""
    n = np.rint(x / (_LN2_HI + _LN2_LO))
    r = ((x - n * _LN2_HI) - n * _LN2_LO) * 0.25
    p = np.full_like(r, 1.0 / 87178291200.0)
    for k in range(13, 0, -1):
        p = p * r + 1.0 / float(np.prod(np.arange(1, k + 1, dtype=np.float64)))
    p = p * r + 1.0
    p = p * p
    return np.ldexp(p * p, n.astype(np.int64))


def _uniform(g, shape):
    """uniform on (-1, 1) from 30-bit integer draws: the same doubles on every machine"""
    return (torch.randint(0, 2 ** 30, shape, generator=g, dtype=torch.int64).double() / 2.0 ** 29 - 1.0).numpy()


def _matvec(k, v):
    out = np.zeros(k.shape[0])
    for col in range(k.shape[1]):  # (fixed order: no BLAS)
        out = out + k[:, col] * v[col]
    return out


def gram(name):
    """(K, z): the RBF-ARD Gram matrix k(Z,Z) = 1.3 exp(-sum_d ((z_d - z'_d) / l_d)^2 / 2) (+ jitter on the diagonal) of the case,
    float64 on the host -- O.RBFARDKernel's formula with exp_reproducible in place of torch.exp"""
    m, d, seed, factor, jitter = CASES[name]
    g = torch.Generator().manual_seed(seed)
    z = _uniform(g, (m, d))
    ls = factor * (0.5 + np.arange(d) / max(d - 1, 1))  # graded: factor * (0.5 .. 1.5)
    d2 = np.zeros((m, m))
    for dim in range(d):
        a = z[:, dim] / ls[dim]
        diff = a[:, None] - a[None, :]
        d2 = d2 + diff * diff
    k = OUTPUTSCALE * exp_reproducible(-0.5 * d2)
    if jitter:
        k = k + jitter * np.eye(m)
    return torch.from_numpy(k), torch.from_numpy(z)


def rhs(name, k, z):
    """(M, 8): three random columns, three u = K v0 with smooth v0 (a rational bump along a random projection of Z: particles
    near the prior mean of a smooth function), two with rough v0 (random signs)"""
    m, d, seed, _, _ = CASES[name]
    g = torch.Generator().manual_seed(seed + 1)
    kn, zn = k.numpy(), z.numpy()
    cols = [_uniform(g, (m,)) for _ in range(3)]
    for i in range(3):
        t = _matvec(zn, _uniform(g, (d,)))
        cols.append(_matvec(kn, 1.0 / (1.0 + (1.0 + i) * (t - 0.3 * i) * (t - 0.3 * i))))
    for _ in range(2):
        cols.append(_matvec(kn, torch.randint(0, 2, (m,), generator=g).double().numpy() * 2 - 1))
    return torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=1)))


def checksum(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    return h.hexdigest()


def load_truth():
    return dict(np.load(TRUTH))


def truth_of(name, file=None):
    """the stored solution as longdouble (hi + lo), after checking that this machine regenerates the very K and U it solves"""
    file = load_truth() if file is None else file
    k, z = gram(name)
    u = rhs(name, k, z)
    assert str(file[f"{name}/sha256"]) == checksum(k, u), \
        f"{name}: k(Z,Z) or U regenerated here differ in some bit from those tests/golden/solve_truth.npz was solved for"
    return k, u, file[f"{name}/hi"].astype(np.longdouble) + file[f"{name}/lo"].astype(np.longdouble)


def _split(a):
    c = np.longdouble(2.0 ** 32 + 1) * a  # Veltkamp: the 64-bit mantissa of a longdouble as two halves of 32 bits
    hi = c - (c - a)
    return hi, a - hi


def residual(kl, x, ul):
    """u - K x for longdouble operands, as if accumulated at twice the precision (Ogita, Rump & Oishi's Dot2: every product
    and every partial sum with its exact error term), then rounded once -- a plain longdouble product would leave the refined
    solution at cond * 2^-64, only 2^-11 below LAPACK's own error"""
    assert np.finfo(np.longdouble).nmant == 63, "the refinement needs the 64-bit mantissa of x87 extended precision"
    s, c = ul.copy(), np.zeros_like(ul)
    for col in range(kl.shape[1]):
        a, b = kl[:, col][:, None], x[col][None, :]
        p = a * b
        (ah, al), (bh, bl) = _split(a), _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # p + e = a b exactly
        t = s - p
        z = t - s
        c += ((s - (t - z)) + (-p - z)) - e  # TwoSum's error term of s - p, and the product's
        s = t
    return s + c


def refined_truth(k, u, sweeps=5):
    """M = 1024: LAPACK's solve refined with residuals at twice longdouble precision.  Returns (solution as longdouble, size
    of the last correction relative to LAPACK's forward error, per column at worst); the caller accepts it below 1e-3."""
    lc = torch.linalg.cholesky(k)
    kl, ul = k.numpy().astype(np.longdouble), u.numpy().astype(np.longdouble)
    x0 = torch.cholesky_solve(u, lc).numpy()
    x = x0.astype(np.longdouble)
    last = None
    for _ in range(sweeps):
        r = residual(kl, x, ul)
        dx = torch.cholesky_solve(torch.from_numpy(r.astype(np.float64)), lc).numpy()
        x = x + dx
        last = np.linalg.norm(dx, axis=0)
    forward = np.linalg.norm((x0 - x).astype(np.float64), axis=0)
    return x, float((last / forward).max())


def errors(k, u, v, truth):
    """per column: forward error |v - v*| / |v*| (2-norms) and backward error |K v - u| / (|K| |v| + |u|) (infinity norms,
    residual in longdouble)"""
    kl, ul = k.numpy().astype(np.longdouble), u.numpy().astype(np.longdouble)
    vl = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v).astype(np.longdouble)
    fwd = np.linalg.norm((vl - truth).astype(np.float64), axis=0) / np.linalg.norm(truth.astype(np.float64), axis=0)
    res = np.abs(residual(kl, vl, ul)).max(axis=0)
    bwd = res / (np.abs(kl).sum(axis=1).max() * np.abs(vl).max(axis=0) + np.abs(ul).max(axis=0))
    return fwd.astype(np.float64), bwd.astype(np.float64)


def host_lapack(lc, u):
    return torch.cholesky_solve(u, lc)


def host_products(lc, u):
    """the product route on the host: Linv by triangular substitution on the identity, then Linv^T (Linv u) in fp64"""
    linv = torch.linalg.solve_triangular(lc, torch.eye(lc.shape[0], dtype=torch.float64), upper=False)
    return linv.T @ (linv @ u)


def host_block_substitution(lc, u, nb=128):
    """The device's substitution route on the host, blocking included (include/plship.h, pls_chol_desc.Sf / Sb): with D_b the
    inverse of the b-th 128 x 128 diagonal block of Lc (triangular substitution on the identity), block row b of the forward
    sweep is ONE product, y_b = [-(D_b Lc[b, :b]), D_b] [y_:b; u_b], and of the backward sweep v_b = [D_b^T, -(Lc[b+:, b] D_b)^T]
    [y_b; v_b+:] -- the operators are formed once, in fp64.  Inside a block this is a product with an inverse, not a
    substitution: for M <= 128 it is the product route itself, and it inherits that route's forward error on right-hand sides
    in the range of K, a block's worth of it."""
    m = lc.shape[0]
    y, v = torch.empty_like(u), torch.empty_like(u)
    blocks = [(b0, min(b0 + nb, m)) for b0 in range(0, m, nb)]
    inv = {b0: torch.linalg.solve_triangular(lc[b0:b1, b0:b1], torch.eye(b1 - b0, dtype=lc.dtype), upper=False) for b0, b1 in blocks}
    for b0, b1 in blocks:
        op = torch.cat([-(inv[b0] @ lc[b0:b1, :b0]), inv[b0]], dim=1)
        y[b0:b1] = op @ torch.cat([y[:b0], u[b0:b1]])
    for b0, b1 in reversed(blocks):
        op = torch.cat([inv[b0].T, -(lc[b1:, b0:b1] @ inv[b0]).T], dim=1)
        v[b0:b1] = op @ torch.cat([y[b0:b1], v[b1:]])
    return v


MARGIN = 8.0


def within(err_device, err_host, m):
    """err_device <= 8 max(err_host, median over the columns of err_host, M 2^-53), per column -> (ok, worst ratio)"""
    bound = np.maximum(np.maximum(err_host, np.median(err_host)), m * 2.0 ** -53)
    ratio = err_device / bound
    return bool((ratio <= MARGIN).all()), float(ratio.max())
