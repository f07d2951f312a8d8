"""GPU: what the train_pls tests of the cost families share (tests/test_gpu_family_cost_train.py, tests/test_gpu_beta_cost_train.py): the
problem on both bases, and one body -- 20 iterations on the reference's host noise stream against
oracle.pls_oracle.train_pls driven by the family's host restatement (the helper and tolerance rule of the small-step parity
tests: test_gpu_parity.step_tolerance, TOL unless the problem itself is ill-conditioned), one launch per iteration, and a
checkpoint saved half way and resumed bit for bit.  A family's truth module states how it draws y, how it builds its host cost and
its library cost from y, and which attribute of the cost the checkpoint carries (train_y, train_costs, CHECKPOINT)."""
import numpy as np
import torch

from oracle import pls_oracle as O
from test_gpu_parity import FUZZ_SEED, build_ipb, build_onb, cu, make_problem, relerr, step_tolerance

SHAPES = [(100, 10, 64), (1000, 32, 100)]  # (N, M, J)
ITERATIONS = 20


def problem(P, n, m, j, base, draw_y, costs):
    """``draw_y(pr, n)``: the family's data from the problem of test_gpu_parity.make_problem; ``costs(P, y)``: (host cost,
    library cost)"""
    pr = make_problem(n, m, j, 2, seed=7 * n + m + FUZZ_SEED)
    y = draw_y(pr, n)
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
    oc, gc = costs(P, y)
    torch.manual_seed(5)
    noises = [ob.sample_update_noise(u0) for _ in range(ITERATIONS)]  # the reference's host stream (torch's generator)
    return ob, gb, oc, gc, u0, eta, noises


def _per_iteration(summary):
    """the kernels a loop launches every iteration; whatever else it launches (entering and leaving the loop's coordinates,
    the whitened operand, the last energies) does not grow with the iterations: a handful per run"""
    named = {k: v for k, v in summary.items() if k != "other"}
    assert all(v["launches"] >= ITERATIONS or v["launches"] <= 4 for v in named.values()), summary
    return {k for k, v in named.items() if v["launches"] >= ITERATIONS}


def training_loop(P, route, tmp_path, n, m, j, base, draw_y, costs, attribute, wrong):
    """``attribute``: the cost parameter that travels with a checkpoint; ``wrong``: a value of it the model the checkpoint is
    loaded into was built with.  Returns the library's cost, for the asserts a family adds of its own."""
    ob, gb, oc, gc, u0, eta, noises = problem(P, n, m, j, base, draw_y, costs)
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
    # a checkpoint half way: the cost's parameter travels with the particles, and the resumed run ends on the same bits
    from projected_langevin_sampling_amd.checkpoint import load_pls, save_pls

    half = ITERATIONS // 2
    mid, e_mid = P.pkg.train_pls(pls, cu(u0).clone(), half, eta, 1e9, noises=dev_noises[:half])
    path = str(tmp_path / "checkpoint.pt")
    save_pls(pls, mid, path, best_lr=eta, number_of_epochs=half)
    other = P.pkg.PLS(gb, costs(P, gc.y_train, wrong)[1])
    assert getattr(other.cost, attribute) != getattr(gc, attribute)
    other, loaded, lr, epochs = load_pls(other, path)
    assert getattr(other.cost, attribute) == getattr(gc, attribute) and lr == eta and epochs == half and torch.equal(loaded, mid)
    end, e_end = P.pkg.train_pls(other, loaded, ITERATIONS - half, eta, 1e9, noises=dev_noises[half:])
    assert torch.equal(end, got) and np.allclose(e_mid + e_end, e_got, rtol=1e-12)
    return gc
