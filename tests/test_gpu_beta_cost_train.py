"""GPU: train_pls with BetaCost under the sigmoid link, on both bases: 20 iterations on the reference's host noise stream
against oracle.pls_oracle.train_pls driven by the host restatement of tests/beta_cost_truth.py (the helper and tolerance rule
of the small-step parity tests: test_gpu_parity.step_tolerance, TOL unless the problem itself is ill-conditioned), one launch
per iteration, and a checkpoint saved half way and resumed bit for bit.  And one run on the in-kernel Philox stream from
particles that put f beyond +-700, against the restatement fed the same normals (oracle/philox_ref.py), with what the bounded
drift implies for the distance from the data-free recursion."""
import math

import numpy as np
import pytest
import torch

import beta_cost_truth as BT
from oracle import philox_ref
from oracle import pls_oracle as O
from test_gpu_parity import FUZZ_SEED, build_ipb, build_onb, cu, make_problem, relerr, step_tolerance
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(100, 10, 64), (1000, 32, 100)]  # (N, M, J): the count-cost shapes
PHI = 8.0
ITERATIONS = 20


def _problem(P, n, m, j, base):
    pr = make_problem(n, m, j, 2, seed=7 * n + m + FUZZ_SEED)
    mu = torch.sigmoid(1.5 * pr["fstar"])  # proportions scattered around sigmoid(1.5 f*) with precision phi
    torch.manual_seed(11 + n)
    y = torch.distributions.Beta(PHI * mu, PHI * (1 - mu)).sample().clamp(1e-6, 1 - 1e-6)
    if base == "onb":
        ob, gb = build_onb(P, pr)
        mk = ob.approximation_dimension
        u0 = 0.1 * pr["u"][:mk].contiguous()
        eta = 0.25 * float(ob.eigenvalues.min())  # inside the stability bound of the stiffest prior mode
    else:
        pr["ls"] = pr["ls"] * 0.35
        ob, gb = build_ipb(P, pr)
        u0 = 0.1 * pr["u"]
        eta = 0.25 * float(torch.linalg.eigvalsh(ob.base_gram_induce).min()) / m
    gc = P.costs.BetaCost(y, P.links.SigmoidLinkFunction(), PHI)
    oc = BT.BetaHostCost(gc.y_device().cpu(), BT.SigmoidLink(), PHI)  # (the very logits the library gets)
    torch.manual_seed(5)
    noises = [ob.sample_update_noise(u0) for _ in range(ITERATIONS)]  # the reference's host stream (torch's generator)
    return ob, gb, oc, gc, u0, eta, noises


def _per_iteration(summary):
    """the kernels a loop launches every iteration; whatever else it launches (entering and leaving the loop's coordinates,
    the whitened operand, the last energies) does not grow with the iterations: a handful per run"""
    named = {k: v for k, v in summary.items() if k != "other"}
    assert all(v["launches"] >= ITERATIONS or v["launches"] <= 4 for v in named.values()), summary
    return {k for k, v in named.items() if v["launches"] >= ITERATIONS}


@pytest.mark.parametrize("base", ["onb", "ipb"])
@pytest.mark.parametrize("n,m,j", SHAPES)
def test_training_loop_against_the_host_restatement(P, route, tmp_path, n, m, j, base):  # noqa: F811
    ob, gb, oc, gc, u0, eta, noises = _problem(P, n, m, j, base)
    assert gc.is_native()
    pls = P.pkg.PLS(gb, gc)
    want, e_want = O.train_pls(O.PLS(ob, oc), u0.clone(), ITERATIONS, eta, 1e9, noises=[x.clone() for x in noises])
    first = O.PLS(ob, oc).calculate_particle_update(u0.clone(), eta, noise=noises[0])
    tol = step_tolerance(ob, oc, u0, eta, noises[0], first)
    route(1)
    dev_noises = [cu(x) for x in noises]
    got, e_got = P.pkg.train_pls(pls, cu(u0).clone(), ITERATIONS, eta, 1e9, noises=dev_noises)
    print(f"{base} {n}x{m}x{j}: particles rel err {relerr(got, want):.3e} (tol {tol:.1e}), energies "
          f"{np.abs(np.array(e_got) / np.array(e_want) - 1).max():.3e}")
    assert len(e_got) == len(e_want) == ITERATIONS
    assert relerr(got, want) < tol
    assert np.allclose(e_got, e_want, rtol=max(tol, 1e-9))
    # one launch per iteration: the step, the energies of its input and their sums in one kernel (the inducing-point basis
    # with injected noise solves in front of it; on its own stream of draws it runs in whitened coordinates, one launch)
    with P.pkg._lib.Timeline(512) as tl:
        P.pkg.train_pls(pls, cu(u0).clone(), ITERATIONS, eta, 1e9, noises=dev_noises)
    assert _per_iteration(tl.summary()) == ({"small_rank_step"} if base == "onb" else {"small_rank_step", "ipb_prep"})
    if base == "ipb":
        with P.pkg._lib.Timeline(512) as tl:
            torch.manual_seed(3)
            P.pkg.train_pls(pls, cu(u0).clone(), ITERATIONS, eta, 1e9)
        assert _per_iteration(tl.summary()) == {"small_rank_step"}
    # a checkpoint half way: the precision travels with the particles, and the resumed run ends on the same bits
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    half = ITERATIONS // 2
    mid, e_mid = P.pkg.train_pls(pls, cu(u0).clone(), half, eta, 1e9, noises=dev_noises[:half])
    path = str(tmp_path / "beta.pt")
    save_pls(pls, mid, path, best_lr=eta, number_of_epochs=half)
    other = P.pkg.PLS(gb, P.costs.BetaCost(gc.y_train, P.links.SigmoidLinkFunction(), 99.0))
    other, loaded, lr, epochs = load_pls(other, path)
    assert other.cost.precision == PHI and lr == eta and epochs == half and torch.equal(loaded, mid)
    end, e_end = P.pkg.train_pls(other, loaded, ITERATIONS - half, eta, 1e9, noises=dev_noises[half:])
    assert torch.equal(end, got) and np.allclose(e_mid + e_end, e_got, rtol=1e-12)


def test_philox_run_from_the_far_tails_keeps_a_bounded_drift(P, route):  # noqa: F811
    """The orthonormal basis, in-kernel Philox noise, started where |f| reaches beyond 700 (exp(-|f|) underflows in part of
    the matrix).  Against the restatement fed the same normals, reproduced on the host.  And the bound that follows from
    |cost'| <= g_max = 1 + phi (0.224 + max|z| / 4) (tests/test_beta_cost_host.py::test_the_drift_is_bounded derives it):
    NOT the 1 + phi |z| / 4 first proposed for this test, which is false for large phi (phi = 400, z = 0: the drift reaches
    88 near f = 1.5); the larger constant asserts less tightly, and it is the smallest closed form that is true:
    with v_t the recursion without the data term on the same normals, d_t = u_t - v_t obeys
    d_(t+1) = (1 - eta / lambda) d_t - eta A G_t with 0 < eta / lambda <= 1/4, so per particle
    |d_T|_2 <= T eta |A|_2 sqrt(N) g_max -- whatever the start."""
    n, m, j, steps = 100, 10, 64, 10
    ob, gb, oc, gc, u0, eta, _ = _problem(P, n, m, j, "onb")
    a = ob.scaled_eigenvectors.T @ ob.base_gram_induce_train  # (M_k, N): F = A^T U
    mk = a.shape[0]
    u0 = u0 * (2000.0 / float((a.T @ u0).abs().max()))
    f0 = a.T @ u0
    assert (f0 > 700).any() and (f0 < -700).any() and (f0.abs() < 30).any()
    torch.manual_seed(3)
    keys = [int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) for _ in range(steps)]  # as the loop draws them
    noises = [torch.from_numpy(philox_ref.normal_matrix(mk, j, key, 0)) for key in keys]
    want, e_want = O.train_pls(O.PLS(ob, oc), u0.clone(), steps, eta, 1e9, noises=[x.clone() for x in noises])
    first = O.PLS(ob, oc).calculate_particle_update(u0.clone(), eta, noise=noises[0])
    tol = step_tolerance(ob, oc, u0, eta, noises[0], first)
    route(1)
    torch.manual_seed(3)
    got, e_got = P.pkg.train_pls(P.pkg.PLS(gb, gc), cu(u0).clone(), steps, eta, 1e9)
    print(f"philox, far start: particles rel err {relerr(got, want):.3e} (tol {tol:.1e})")
    assert len(e_got) == steps and all(math.isfinite(e) for e in e_got) and torch.isfinite(got).all()
    assert relerr(got, want) < tol and np.allclose(e_got, e_want, rtol=max(tol, 1e-9))
    v = u0.clone()
    shrink = (1 - eta / ob.eigenvalues)[:, None]
    assert (shrink >= 0.75).all() and (shrink < 1).all()
    for xi in noises:
        v = shrink * v + math.sqrt(2 * eta) * xi
    g_max = (1 + PHI * (0.224 + float(oc.z_train.abs().max()) / 4)) * (1 + 2.0 ** -40)
    bound = steps * eta * float(torch.linalg.matrix_norm(a, 2)) * math.sqrt(n) * g_max
    dist = torch.linalg.vector_norm(got.cpu() - v, dim=0)
    print(f"philox, far start: |u_T - v_T| max {dist.max().item():.3e}, bound {bound:.3e}")
    assert (dist <= bound).all()
    # the derivative the run started from is within g_max everywhere, and +-1 up to phi |z| e^-700 where |f| > 700
    g0 = gc.calculate_cost_derivative(cu(f0)).cpu()
    assert (g0.abs() <= g_max).all() and (g0[f0.abs() > 700].abs() == 1).all()
