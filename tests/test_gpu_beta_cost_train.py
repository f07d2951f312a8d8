"""GPU: train_pls with BetaCost under the sigmoid link, next to the loop every family runs
(tests/test_gpu_family_cost_train.py), on the problem of tests/train_loop_fixtures.py: one run on the in-kernel Philox stream
from particles that put f beyond +-700, against the restatement fed the same normals (oracle/philox_ref.py), with what the
bounded drift implies for the distance from the data-free recursion."""
import math

import numpy as np
import pytest
import torch

import beta_cost_truth as BT
from oracle import philox_ref
from oracle import pls_oracle as O
from test_gpu_parity import cu, relerr, step_tolerance
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)
from train_loop_fixtures import problem

pytestmark = pytest.mark.gpu

PHI = BT.TRAIN_PRECISION


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
    ob, gb, oc, gc, u0, eta, _ = problem(P, n, m, j, "onb", BT.train_y, BT.train_costs)
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
