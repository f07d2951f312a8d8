"""GPU: libplship's symmetric eigensolver (pls_sym_eigh: blocked two-sided Jacobi, csrc/sym_eigh.hip) against 50-digit
truth (tests/golden/sym_eigh_truth.npz) and LAPACK, and the eigh_device="plship" route through the package.

Bars.  Per case the residual max|A V - V L| and the eigenvalue error must stay within 4 M eps ||A||_2 and the
orthogonality max|V^T V - I| within 4 M eps, all evaluated in np.longdouble.  That is a cap, not a measurement: what it
must not hide -- a stop that is too early, a pair left out of the schedule, a padding row mixed in -- leaves errors of
1e-10 and more, far above 4 M eps <= 5e-13 at these sizes, and LAPACK alone stays within it on all these inputs (1 to 4
eps for residual and eigenvalues, 7 to 17 eps for orthogonality).  PLS_SYM_EIGH_DUMP=<path> writes the measured maxima, and
LAPACK's on the same inputs, to that file (profiles/sym_eigh_accuracy.txt is such a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sym_eigh_truth as T

pytestmark = pytest.mark.gpu

# 64: the last single-launch size; 65 pads by 31; 96 = three blocks (a bye per round); 97, 128: two pairs per round;
# 520: 17 blocks
SIZES = (1, 2, 3, 17, 63, 64, 65, 96, 97, 128, 130, 200, 257, 520)
LD = np.longdouble


@pytest.fixture(scope="module")
def ops():
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd import _ops

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg._lib.load()
    return _ops


@pytest.fixture(scope="module")
def records():
    rows = []
    yield rows
    path = os.environ.get("PLS_SYM_EIGH_DUMP")
    if path and rows:
        with open(path, "w") as f:
            f.write("# pls_sym_eigh accuracy (tests/test_gpu_sym_eigh.py), in units of eps * scale; scale = ||A||_2 for the residual\n"
                    "# max|A V - V L| and the eigenvalue error, 1 for the orthogonality max|V^T V - I|; the cap is 4 M.  Evaluated in\n"
                    "# np.longdouble; eigenvalue reference: mpmath (50 digits) where the fixture has the case, else LAPACK\n"
                    "# (numpy.linalg.eigvalsh).  'lapack' columns: numpy.linalg.eigh on the same input.\n")
            f.write(f"{'case':<22}{'M':>5}{'ref':>8}{'cap':>7} | {'res':>8}{'orth':>8}{'eig':>8} | {'res':>8}{'orth':>8}{'eig':>8}  (plship | lapack)\n")
            for r in rows:
                f.write(f"{r['case']:<22}{r['m']:>5}{r['ref']:>8}{4 * r['m']:>7} | {r['res']:>8.2f}{r['orth']:>8.2f}{r['eig']:>8.2f} | "
                        f"{r['res_l']:>8.2f}{r['orth_l']:>8.2f}{r['eig_l']:>8.2f}\n")
            worst = max(rows, key=lambda r: max(r["res"] / max(r["res_l"], 1), r["orth"] / max(r["orth_l"], 1)))
            f.write(f"# largest ratio to LAPACK's own figure (floored at 1 eps): {worst['case']} M = {worst['m']}\n")


def solve(ops, a):
    lam, vec, info = ops.sym_eigh(torch.from_numpy(np.ascontiguousarray(a)).cuda(), return_info=True)
    torch.cuda.synchronize()
    return lam.cpu().numpy(), vec.cpu().numpy(), info


def measures(a, lam, vec, lam_ref):
    """(residual, orthogonality, eigenvalue error) in units of eps * scale; longdouble arithmetic."""
    m = a.shape[0]
    scale = float(np.abs(lam_ref).max()) if m else 0.0  # ||A||_2 of a symmetric matrix
    al, vl, ll = a.astype(LD), vec.astype(LD), lam.astype(LD)
    res = float(np.abs(al @ vl - vl * ll[None, :]).max())
    orth = float(np.abs(vl.T @ vl - np.eye(m, dtype=LD)).max())
    eig = float(np.abs(ll - lam_ref.astype(LD)).max())
    unit = T.EPS * scale
    if unit == 0.0:
        return (0.0 if res == 0 else np.inf), orth / T.EPS, (0.0 if eig == 0 else np.inf)
    return res / unit, orth / T.EPS, eig / unit


def check_case(ops, records, name, a, lam_ref, ref, eigenvalues_only_by_residual=False):
    m = a.shape[0]
    lam, vec, info = solve(ops, a)
    assert info == 0, f"{name} M = {m}: not converged"
    assert np.all(np.diff(lam) >= 0), "ascending"
    pivot = np.abs(vec).argmax(axis=0)  # first maximal index per column
    assert np.all(vec[pivot, np.arange(m)] > 0), "sign rule"
    res, orth, eig = measures(a, lam, vec, lam_ref)
    ll, vl = np.linalg.eigh(a)
    res_l, orth_l, eig_l = measures(a, ll, vl, lam_ref)
    records.append(dict(case=name, m=m, ref=ref, res=res, orth=orth, eig=eig, res_l=res_l, orth_l=orth_l, eig_l=eig_l))
    print(f"{name} M={m}: res {res:.2f} orth {orth:.2f} eig {eig:.2f} (lapack {res_l:.2f} {orth_l:.2f} {eig_l:.2f}) cap {4 * m}")
    cap = 4 * m
    assert res <= cap, f"{name} M = {m}: residual {res:.1f} eps ||A||_2 > {cap}"
    assert orth <= cap, f"{name} M = {m}: orthogonality {orth:.1f} eps > {cap}"
    assert eig <= cap, f"{name} M = {m}: eigenvalue error {eig:.1f} eps ||A||_2 > {cap}"
    return lam, vec


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("family", T.FAMILIES)
def test_families(ops, records, family, m):
    a, lam_ref, ref = T.case(family, m)
    check_case(ops, records, family, a, lam_ref, ref)


@pytest.mark.parametrize("m", (17, 96))
def test_zero_diagonal_and_identity(ops, records, m):
    lam, vec = check_case(ops, records, "zero", np.zeros((m, m)), np.zeros(m), "exact")
    assert np.all(lam == 0) and np.array_equal(vec, np.eye(m))
    d = np.random.default_rng(m).standard_normal(m)  # unsorted: no rotation, a permutation
    lam, vec = check_case(ops, records, "diagonal", np.diag(d), np.sort(d), "exact")
    assert np.array_equal(lam, np.sort(d))
    assert np.array_equal(vec, np.eye(m)[:, np.argsort(d, kind="stable")])
    lam, vec = check_case(ops, records, "c * I", 0.37 * np.eye(m), np.full(m, 0.37), "exact")
    assert np.all(lam == 0.37)


@pytest.mark.parametrize("m", (17, 130))
@pytest.mark.parametrize("scale", (1e150, 1e-150))
def test_extreme_scales(ops, records, m, scale):
    a = T.case("rbf", m)[0] * scale
    check_case(ops, records, f"rbf * {scale:g}", a, np.linalg.eigvalsh(a), "lapack")


@pytest.mark.parametrize("m", (40, 130))
def test_same_bits_twice_upper_triangle_unread_input_unchanged(ops, m):
    a = T.make_matrix("indef", m)
    dev = torch.from_numpy(a).cuda()
    keep = dev.clone()
    first = ops.sym_eigh(dev)
    second = ops.sym_eigh(dev)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(dev, keep), "A is not written"
    dirty = a.copy()
    dirty[np.triu_indices(m, 1)] = np.nan
    third = ops.sym_eigh(torch.from_numpy(dirty).cuda())
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


@pytest.mark.parametrize("m", (40, 130))
def test_leading_dimensions_and_guards(ops, m):
    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    lib = L.load()
    a = T.make_matrix("matern12", m)
    want = ops.sym_eigh(torch.from_numpy(a).cuda())
    lda, ldv, guard = m + 5, m + 3, -7.25
    big = torch.full((m, lda), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :m] = torch.from_numpy(a).cuda()
    vbuf = torch.full((m + 2, ldv), guard, dtype=torch.float64, device="cuda")
    lbuf = torch.full((m + 4,), guard, dtype=torch.float64, device="cuda")
    nbytes = lib.pls_sym_eigh_workspace_bytes(m)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device="cuda")
    ws[-2:] = guard
    info = C.c_int32(-1)
    v0 = vbuf[1:].reshape(-1)  # V starts one row in: a guard row before and after
    L.check(lib.pls_sym_eigh(big.data_ptr(), lda, m, lbuf[2:].data_ptr(), vbuf[1:].data_ptr(), ldv, C.byref(info), ws.data_ptr(),
                             nbytes, L.stream_ptr()), "pls_sym_eigh")
    torch.cuda.synchronize()
    assert info.value == 0
    assert torch.equal(lbuf[2:m + 2], want[0]) and torch.equal(vbuf[1:m + 1, :m], want[1])
    assert bool((lbuf[:2] == guard).all()) and bool((lbuf[m + 2:] == guard).all())
    assert bool((vbuf[0] == guard).all()) and bool((vbuf[m + 1] == guard).all()) and bool((vbuf[1:m + 1, m:] == guard).all())
    assert bool((ws[-2:] == guard).all()) and v0.numel() > 0


@pytest.mark.parametrize("m", (9, 130))
def test_non_finite_input_is_refused(ops, m):
    import projected_langevin_sampling_amd as pkg

    a = T.make_matrix("rbf", m)
    a[m - 1, 2] = np.nan  # the lower triangle
    with pytest.raises(pkg._lib.PlsHipError, match="non-finite"):
        ops.sym_eigh(torch.from_numpy(a).cuda())
    a[m - 1, 2] = np.inf
    with pytest.raises(pkg._lib.PlsHipError, match="non-finite"):
        ops.sym_eigh(torch.from_numpy(a).cuda())


# ------------------------------------------------------------------------------------------------------------
# through the package: eigh_device="plship"
# ------------------------------------------------------------------------------------------------------------
def relerr(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _problem(n, m, j, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g, dtype=torch.float64) * 2 - 1
    z = x[torch.randperm(n, generator=g)[:m]].clone()
    y = torch.sin(2.0 * (x @ torch.randn(d, generator=g, dtype=torch.float64))) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=torch.float64)) * 0.6
    return x, z, y, ls, g


@pytest.mark.parametrize("m", (30, 200))
def test_orthonormal_basis_on_the_plship_route(ops, m):
    """The comparison and the bars of tests/test_gpu_parity.py::test_eigh_on_the_gpu_gives_the_same_basis_up_to_the_gauge:
    the kept count, the eigenvalues (1e-10) and the gauge-invariant operator A^T diag(lam) A (1e-8); and one Gaussian step
    from the same particles, compared in function space (the particles are the same FUNCTIONS in both gauges)."""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.basis import OrthonormalBasis
    from projected_langevin_sampling_amd.costs import GaussianCost
    from projected_langevin_sampling_amd.link_functions import IdentityLinkFunction

    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x, z, y, ls, g = _problem(400, m, 8, 3, seed=21)
        gk = pkg.ARDKernel(ls, 1.3)
        bases = [OrthonormalBasis(pkg.PLSKernel(gk, z), z, x, 1e-10, verbose=False, eigh_device=dev) for dev in ("cpu", "plship")]
        assert bases[0].approximation_dimension == bases[1].approximation_dimension
        assert relerr(bases[1].eigenvalues, bases[0].eigenvalues) < 1e-10
        ops_ = [(b._A.T * b.eigenvalues[None, :]) @ b._A for b in bases]
        assert relerr(ops_[1], ops_[0]) < 1e-8
        # the same FUNCTION in both gauges: u = diag(lam) A w for one coefficient vector w in data space gives
        # f = A^T diag(lam) A w, the gauge-invariant operator above applied to w
        mk = bases[0].approximation_dimension
        w = torch.randn(400, 8, generator=g, dtype=torch.float64).cuda()
        starts = [b.eigenvalues[:, None] * (b._A @ w) for b in bases]
        f0 = [b._A.T @ u for b, u in zip(bases, starts)]
        assert relerr(f0[1], f0[0]) < 1e-8
        xi = torch.zeros(mk, 8, dtype=torch.float64).cuda()
        new_f = []
        for b, u in zip(bases, starts):
            step = pkg.PLS(b, GaussianCost(0.3, y, IdentityLinkFunction())).calculate_particle_update(u, 1e-3, noise=xi)
            new_f.append(b._A.T @ (u + step))
        assert relerr(new_f[1], new_f[0]) < 1e-8
    finally:
        torch.set_default_dtype(prev)


def test_spectral_factor_of_an_indefinite_covariance(ops):
    from projected_langevin_sampling_amd import samplers

    cov = torch.from_numpy(T.make_matrix("indef", 140)).cuda()
    f_cpu = samplers.spectral_factor(cov, "cpu")
    f_own = samplers.spectral_factor(cov, "plship")
    assert f_own.shape == (140, 140)
    clipped = [f.T @ f for f in (f_cpu, f_own)]  # Q max(L, 0) Q^T: gauge invariant
    assert relerr(clipped[1], clipped[0]) < 1e-8
    lam = np.linalg.eigvalsh(cov.cpu().numpy())
    assert lam[0] < -1e-3 * lam[-1], "the case is indefinite"


@pytest.mark.parametrize("m", (30, 200))
def test_shared_spectrum_returns_canonical_signs(ops, m):
    from projected_langevin_sampling_amd.basis.spectrum import canonicalise_signs, shared_spectrum

    g = torch.from_numpy(T.make_matrix("rbf", m)).cuda()
    lam, vec = shared_spectrum(g, "plship")
    assert lam.device.type == "cpu" and vec.shape == (m, m)
    assert torch.equal(canonicalise_signs(vec), vec)
    lam_c, _ = shared_spectrum(g, "cpu")
    assert relerr(lam, lam_c) < 1e-10
