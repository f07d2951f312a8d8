"""CPU: the SVGP yardstick (tests/svgp_truth.py) against autograd, against its 50-digit fixture and against the closed-form
optimum; the epoch's index batches against a shuffled loader over the data; the options that are not supported."""
import ctypes

import numpy as np
import pytest
import torch

import svgp_truth as T


def _autograd_vector(inp):
    mean = inp["mean"].clone().requires_grad_(True)
    Ls = inp["Ls"].clone().requires_grad_(True)
    c = torch.tensor(inp["c"], dtype=torch.float64, requires_grad=True)
    rho = torch.tensor(inp["rho"], dtype=torch.float64, requires_grad=True)
    elbo = T.elbo_torch(inp["At"], inp["q"], inp["y"], mean, Ls, c, rho, inp["idx"], inp["n"])
    elbo.backward()
    return elbo.item(), c.grad.item(), rho.grad.item(), mean.grad.numpy(), T.lower_entries(Ls.grad.numpy()), Ls.grad


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_hand_derived_gradients_equal_autograd(name):
    inp, out, scale = T.cpu_case(name)
    m, b, _ = T.CASES[name]
    elbo, g_c, g_rho, g_m, g_l, full = _autograd_vector(inp)
    got = np.concatenate([[elbo, g_c, g_rho], g_m, g_l])
    want = np.concatenate([out[:3], out[5:]])
    s = np.concatenate([scale[:3], scale[5:]])
    err = np.abs(got - want) / s
    print(f"{name}: worst |hand - autograd| / S = {err.max():.2e}, bar {T.bar(m, b):.2e}")
    assert (err <= T.bar(m, b)).all()
    assert torch.equal(torch.triu(full, diagonal=1), torch.zeros_like(full))  # nothing above the diagonal enters
    # the vectorised formulas the SGD loop uses
    fast = T.gradients_torch(inp["At"], inp["q"], inp["y"], inp["mean"], inp["Ls"], torch.tensor(inp["c"], dtype=torch.float64),
                             torch.tensor(inp["rho"], dtype=torch.float64), inp["idx"], inp["n"])
    got = np.concatenate([[fast[0].item(), fast[3].item(), fast[4].item()], fast[1].numpy(), T.lower_entries(fast[2].numpy())])
    assert (np.abs(got - want) / s <= T.bar(m, b)).all()


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_float64_evaluation_against_the_50_digit_truth(name):
    _, out, scale = T.cpu_case(name)
    m, b, _ = T.CASES[name]
    hi, lo = T.truth(name)
    assert hi.shape == out.shape == (5 + m + m * (m + 1) // 2,)
    err = T.relative_error(out, hi, lo, scale)
    print(f"{name}: worst |fsum - truth| / S = {err.max():.2e}, bar {T.bar(m, b):.2e}")
    assert (err <= T.bar(m, b)).all()


def test_the_majorant_dominates_every_output():
    for name in ("m17-b63", "m33-b65", "m1-b1"):
        _, out, scale = T.cpu_case(name)
        assert (scale >= np.abs(out)).all() and (scale > 0).all()


@pytest.mark.parametrize("n,batch_size", [(10, 3), (65, 65), (200, 64), (7, 100)])
def test_epoch_batches_select_the_rows_of_a_shuffled_loader(n, batch_size):
    from torch.utils.data import DataLoader, TensorDataset

    from projected_langevin_sampling_amd.trainers import epoch_batches
    from projected_langevin_sampling_amd.utils import set_seed

    x = torch.arange(3 * n, dtype=torch.float64).reshape(n, 3) * 0.5
    y = -torch.arange(n, dtype=torch.float64)
    set_seed(11)
    torch.randn(5)  # (the variational mean is drawn before the loader exists)
    loader = DataLoader(TensorDataset(x, y), batch_size=batch_size, shuffle=True)
    want = [[(xb, yb) for xb, yb in loader] for _ in range(2)]  # two epochs of one loader
    set_seed(11)
    torch.randn(5)
    for epoch in want:
        got = epoch_batches(n, batch_size)
        assert len(got) == len(epoch) == -(-n // batch_size)
        for idx, (xb, yb) in zip(got, epoch):
            assert idx.dtype == torch.int64 and torch.equal(x[idx], xb) and torch.equal(y[idx], yb)
        assert got[-1].numel() == n - (len(got) - 1) * batch_size  # the ragged last batch
        assert sorted(torch.cat(got).tolist()) == list(range(n))


@pytest.mark.parametrize("n,m", [(40, 3), (200, 17)])
def test_gradients_vanish_at_the_closed_form_optimum(n, m):
    """an independent check of the bound itself: at S* = (I + A A^T / sigma^2)^-1, m* = S* A (y - c) / sigma^2 the
    full-batch gradients with respect to m and L_s are zero up to the rounding of their terms"""
    inp = T.make_inputs(31000 + m, n, m)
    m_star, l_star = T.closed_form_optimum(inp["At"], inp["y"], inp["c"], inp["rho"])
    inp.update(mean=m_star, Ls=l_star)
    out, scale = T.evaluate_inputs(inp), T.evaluate_inputs(inp, majorant=True)
    err = np.abs(out[5:]) / scale[5:]
    print(f"n={n} m={m}: worst |gradient| / S at the optimum = {err.max():.2e}, bar {T.bar(m, n):.2e}")
    assert (err <= T.bar(m, n)).all()
    # and it IS the optimum: the ELBO drops along any direction
    for k in range(3):
        moved = dict(inp, mean=m_star + 1e-3 * T._normal(torch.Generator().manual_seed(k), (m,)))
        assert T.evaluate_inputs(moved)[0] < out[0]


def test_unsupported_options_raise():
    import projected_langevin_sampling_amd as pkg

    z = torch.zeros(4, 2)
    kernel = pkg.ARDKernel([1.0, 1.0], 1.0)
    with pytest.raises(NotImplementedError, match="learn_inducing_locations.*fixed"):
        pkg.SVGP(kernel, z, learn_inducing_locations=True)
    for likelihood in ("bernoulli", "student_t"):
        with pytest.raises(NotImplementedError, match="only 'gaussian'"):
            pkg.SVGP(kernel, z, likelihood=likelihood)
    with pytest.raises(NotImplementedError, match="learn_kernel_parameters.*fixed"):
        pkg.train_svgp(torch.zeros(8, 2), torch.zeros(8), z, kernel, 0, 1, 4, 0.1, 1e-4, learn_kernel_parameters=True)
    with pytest.raises(NotImplementedError, match="learn_inducing_locations"):
        pkg.train_svgp(torch.zeros(8, 2), torch.zeros(8), z, kernel, 0, 1, 4, 0.1, 1e-4, learn_inducing_locations=True)
    with pytest.raises(ValueError, match="257 inducing points"):
        pkg.SVGP(kernel, torch.zeros(257, 2))


def test_cabi_rejects_what_it_does_not_support():
    """validation happens before any HIP call: another likelihood, more than 256 inducing points, a short workspace"""
    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    lib = L.load()

    def desc(m=8, likelihood=L.SVGP_GAUSSIAN):
        d = L.SvgpDesc()
        d.At, d.ldat, d.q, d.y, d.n, d.m, d.likelihood = 8, m, 8, 8, 64, m, likelihood
        return d

    def call(d, ws_bytes=1 << 30):
        return lib.pls_svgp_elbo_grad(ctypes.byref(d), 8, 8, d.m, 8, None, 64, 8, 8, 8, d.m, 8, ws_bytes, None)

    assert call(desc(likelihood=1)) == 1 and b"PLS_SVGP_GAUSSIAN only" in lib.pls_last_error()
    assert call(desc(m=257)) == 1 and b"257 inducing points > 256" in lib.pls_last_error()
    assert call(desc(), ws_bytes=16) == 3 and b"needed" in lib.pls_last_error()
    assert lib.pls_svgp_workspace_bytes(1000, 100, 1000) == 8 * (4 + 4 * 32 + 32 * 112 * 113)
    assert lib.pls_svgp_workspace_bytes(36000, 16, 32) == 8 * (4 + 4 * 1125)
    assert lib.pls_svgp_workspace_bytes(10, 257, 10) == 0
    assert ctypes.sizeof(L.SvgpDesc) == 7 * 8
