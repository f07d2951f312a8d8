"""GPU: the SVGP entries of libplship (csrc/svgp.hip) -- every output of pls_svgp_elbo_grad against the 50-digit fixture and
the fsum helper within (M + B + 16) eps S, the bit-for-bit equalities the header promises, pls_svgp_sgd_epoch against its
replay, train_svgp against the helper's CPU loop, prediction, TemperGP and the whole chain on the library alone.

Shapes: the kernels tile the points by 32 and the inducing points by 16, four waves take the 16-column tiles in turn (a
round of 64 columns): M and B sit at 1, 2 and one below / at / one above those edges."""
import ctypes

import numpy as np
import pytest
import torch

import svgp_truth as T

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")


class Dev:
    """the inputs of svgp_truth.make_inputs on the device, every buffer padded with NaN: the padding columns of At, the
    upper triangle and the padding of L_s, and a tail behind every output"""

    TAIL = 3

    def __init__(self, inp, ls_offset=0):
        import projected_langevin_sampling_amd as pkg

        self.L = L = pkg._lib
        self.lib = L.load()
        self.inp = inp
        At = inp["At"]
        self.n, self.m = At.shape
        n, m = self.n, self.m
        self.ldat = m + 2
        at = torch.full((n, self.ldat), NAN, dtype=F64)
        at[:, :m] = At
        self.at = at.cuda()
        self.q, self.y, self.mean = inp["q"].cuda(), inp["y"].cuda(), inp["mean"].cuda()
        self.ldls = m + 1
        ls = torch.full((m * self.ldls + 2,), NAN, dtype=F64)
        body = ls[ls_offset:ls_offset + m * self.ldls].view(m, self.ldls)
        k, l = np.tril_indices(m)
        body[k, l] = inp["Ls"][k, l]
        self.ls_buf = ls.cuda()
        self.ls = self.ls_buf[ls_offset:ls_offset + m * self.ldls].view(m, self.ldls)
        self.scalars = torch.tensor([inp["c"], inp["rho"]], dtype=F64).cuda()
        self.desc = L.SvgpDesc()
        self.desc.At, self.desc.ldat, self.desc.q, self.desc.y = self.at.data_ptr(), self.ldat, self.q.data_ptr(), self.y.data_ptr()
        self.desc.n, self.desc.m, self.desc.likelihood = n, m, L.SVGP_GAUSSIAN
        self.tril = (torch.from_numpy(k).cuda(), torch.from_numpy(l).cuda())
        nbytes = self.lib.pls_svgp_workspace_bytes(n, m, n)
        self.ws = torch.full((nbytes // 8 + 2,), NAN, dtype=F64, device="cuda")
        self.ws_bytes = nbytes

    def evaluate(self, idx="case", gradients=True):
        """one pls_svgp_elbo_grad call -> (out (5), grad_m (M), grad_L (M, M+1 with its padding)); sentinels checked"""
        m, L = self.m, self.L
        if isinstance(idx, str):
            idx = self.inp["idx"]
        b = self.n if idx is None else idx.numel()
        idx_dev = None if idx is None else idx.cuda()
        out = torch.full((5 + self.TAIL,), NAN, dtype=F64, device="cuda")
        gm = torch.full((m + self.TAIL,), NAN, dtype=F64, device="cuda")
        gl = torch.full((m, m + 1), NAN, dtype=F64, device="cuda")
        before = self.ls_buf.clone()
        L.check(self.lib.pls_svgp_elbo_grad(ctypes.byref(self.desc), self.mean.data_ptr(), self.ls.data_ptr(), self.ldls,
                                            self.scalars.data_ptr(), L.ptr(idx_dev), b, out.data_ptr(),
                                            gm.data_ptr() if gradients else None, gl.data_ptr() if gradients else None, m + 1,
                                            self.ws.data_ptr(), self.ws_bytes, L.stream_ptr()), "pls_svgp_elbo_grad")
        torch.cuda.synchronize()
        assert torch.isnan(out[5:]).all() and torch.isnan(gm[m:]).all(), "a sentinel behind an output was overwritten"
        assert torch.isnan(self.ws[self.ws_bytes // 8:]).all(), "the workspace was overrun"
        assert torch.equal(self.ls_buf.view(torch.int64), before.view(torch.int64)), "L_s was written"
        if gradients:
            upper = torch.triu(torch.ones(m, m + 1, dtype=torch.bool, device="cuda"), diagonal=1)
            assert torch.isnan(gl[upper]).all(), "grad_L was written above the diagonal"
        else:
            assert torch.isnan(gm).all() and torch.isnan(gl).all()
        return out[:5], gm[:m], gl

    def vector(self, out, gm, gl):
        return torch.cat([out, gm, gl[self.tril[0], self.tril[1]]]).cpu().numpy()


def _check(name, got, want_hi, want_lo, scale, m, b):
    err = T.relative_error(got, want_hi, want_lo, scale)
    worst = int(np.argmax(err))
    print(f"{name}: worst |device - truth| / S = {err.max():.2e} at output {worst} (bar {T.bar(m, b):.2e})")
    assert np.isfinite(got).all()
    assert (err <= T.bar(m, b)).all()


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_every_output_against_the_50_digit_truth(name):
    inp, _, scale = T.cpu_case(name)
    m, b, _ = T.CASES[name]
    hi, lo = T.truth(name)
    dev = Dev(inp)
    _check(name, dev.vector(*dev.evaluate()), hi, lo, scale, m, b)


LARGER = [(15, 31), (16, 32), (17, 33), (31, 64), (32, 65), (33, 63), (63, 130), (64, 2), (65, 1), (130, 33), (191, 130), (256, 65)]
_larger_cache = {}


def _larger(m, b):
    if (m, b) not in _larger_cache:
        inp = T.make_inputs(810000 + 1000 * m + b, 300, m, b)
        _larger_cache[(m, b)] = (inp, T.evaluate_inputs(inp), T.evaluate_inputs(inp, majorant=True))
    return _larger_cache[(m, b)]


@pytest.mark.parametrize("m,b", LARGER)
def test_every_output_against_the_fsum_helper(m, b):
    inp, want, scale = _larger(m, b)
    dev = Dev(inp)
    _check(f"m{m}-b{b}", dev.vector(*dev.evaluate()), want, np.zeros_like(want), scale, m, b)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("m,b", [(17, 65), (65, 33), (191, 130)])
def test_bit_for_bit_equalities(m, b):
    inp, _, _ = _larger(m, b) if (m, b) in LARGER else (T.make_inputs(820000 + m, 300, m, b), None, None)
    dev = Dev(inp)

    def same(r1, r2):
        k, l = dev.tril
        return all(torch.equal(_bits(x), _bits(y)) for x, y in ((r1[0], r2[0]), (r1[1], r2[1]), (r1[2][k, l], r2[2][k, l])))

    first = dev.evaluate()
    assert same(first, dev.evaluate()), "two calls differ"
    # NULL idx = the identity list (on the first b rows as the whole data set)
    ident = torch.arange(b, dtype=torch.int64)
    head = dict(inp, At=inp["At"][:b], q=inp["q"][:b], y=inp["y"][:b], n=b)
    part = Dev(head).evaluate(idx=ident)
    assert same(Dev(head).evaluate(idx=None), part), "NULL idx and the identity list differ"
    # the same rows inside the larger data set differ only through KL / n: (1/B) sum l_i and KL are the same bits
    assert torch.equal(_bits(dev.evaluate(idx=ident)[0][3:5]), _bits(part[0][3:5]))
    # the value-only kernel
    assert torch.equal(_bits(dev.evaluate(gradients=False)[0]), _bits(first[0]))
    # L_s at an odd offset (8-byte aligned only): there is one load path, the bits are the same
    assert same(first, Dev(inp, ls_offset=1).evaluate())


@pytest.mark.parametrize("n,m,batch_size,flags", [(150, 17, 64, 3), (150, 17, 64, 1), (150, 17, 64, 2), (100, 65, 33, 3),
                                                  (70, 130, 70, 0)])
def test_the_epoch_equals_its_replay(n, m, batch_size, flags):
    """pls_svgp_sgd_epoch over a shuffled perm (ragged last batch) = pls_svgp_elbo_grad per batch + p - lr * (-g) by torch,
    bit for bit in m, tril L_s, c and rho; a frozen scalar keeps its bits; loss_out = - the value-only ELBO on all rows"""
    lr = 0.05
    inp = T.make_inputs(830000 + m, n, m)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n + m))
    dev, rep = Dev(inp), Dev(inp)
    L = dev.L
    loss = torch.full((1 + Dev.TAIL,), NAN, dtype=F64, device="cuda")
    perm_dev = perm.cuda()
    L.check(dev.lib.pls_svgp_sgd_epoch(ctypes.byref(dev.desc), dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls,
                                       dev.scalars.data_ptr(), perm_dev.data_ptr(), batch_size, lr, flags, loss.data_ptr(),
                                       dev.ws.data_ptr(), dev.ws_bytes, L.stream_ptr()), "pls_svgp_sgd_epoch")
    torch.cuda.synchronize()
    k, l = rep.tril
    for first in range(0, n, batch_size):
        out, gm, gl = rep.evaluate(idx=perm[first:first + batch_size])
        rep.mean.copy_(rep.mean - lr * (-gm))
        rep.ls[k, l] = rep.ls[k, l] - lr * (-gl[k, l])
        if flags & L.SVGP_TRAIN_MEAN:
            rep.scalars[0] = rep.scalars[0] - lr * (-out[1])
        if flags & L.SVGP_TRAIN_NOISE:
            rep.scalars[1] = rep.scalars[1] - lr * (-out[2])
    assert torch.equal(_bits(dev.mean), _bits(rep.mean))
    assert torch.equal(_bits(dev.ls_buf), _bits(rep.ls_buf))  # (the NaN upper triangle and padding included)
    assert torch.equal(_bits(dev.scalars), _bits(rep.scalars))
    start = torch.tensor([inp["c"], inp["rho"]], dtype=F64)
    moved = _bits(dev.scalars.cpu()) != _bits(start)
    assert moved.tolist() == [bool(flags & 1), bool(flags & 2)]
    assert not torch.equal(_bits(dev.mean.cpu()), _bits(inp["mean"]))
    value = rep.evaluate(idx=None, gradients=False)[0]
    assert torch.isnan(loss[1:]).all() and torch.isfinite(loss[0])
    assert torch.equal(_bits(loss[:1]), _bits(-value[:1]))
    assert torch.isnan(dev.ws[dev.ws_bytes // 8:]).all()


def _data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g, dtype=F64) * 2 - 1
    y = torch.sin(3 * x.sum(dim=1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)
    return x, y


def test_training_follows_the_cpu_loop():
    """train_svgp (one library call per epoch) against the helper's loop on the same batches and the same whitened rows.
    The bar comes from the CPU loop alone: rerun with every gradient component perturbed by a relative 1e-12 (alternating
    signs), 16 x the divergence of the losses and of the final parameters, floor 1e-11."""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.utils import set_seed

    n, m, bs, epochs, lr, seed = 300, 17, 65, 30, 0.02, 4
    x, y = _data(n, 2, 41)
    z = x[:m].clone()
    kernel = pkg.PLSKernel(pkg.ARDKernel([0.6, 0.8], 1.2), z)
    model, losses = pkg.train_svgp(x, y, z, kernel, seed, epochs, bs, lr, early_stopper_patience=1e9)
    assert model is not None and len(losses) == epochs
    set_seed(seed)
    mean0 = 1e-3 * torch.randn(m, dtype=F64)
    batches = [pkg.epoch_batches(n, bs) for _ in range(epochs)]
    assert [b.numel() for b in batches[0]] == [65, 65, 65, 65, 40]
    st = model._dev
    At, q = st["At"].cpu().contiguous(), st["q"].cpu()
    assert (q > 0).all()
    args = (At, q, y, mean0, torch.eye(m, dtype=F64), 0.0, 0.0, batches, lr)
    cpu = T.sgd_loop(*args)
    per = T.sgd_loop(*args, perturb=1e-12)
    k, l = np.tril_indices(m)

    def params(mean, ls, c, rho):
        return np.concatenate([np.asarray(mean), np.asarray(ls)[k, l], [c, rho]])

    p_cpu, p_per = params(*cpu[1:]), params(*per[1:])
    p_gpu = params(model.variational_mean.cpu(), model.chol_variational_covar.cpu(), *model.scalars.cpu().tolist())
    bar_loss = max(16.0 * np.abs(np.array(cpu[0]) - np.array(per[0])).max(), 1e-11)
    bar_par = max(16.0 * np.abs(p_cpu - p_per).max(), 1e-11)
    d_loss, d_par = np.abs(np.array(cpu[0]) - np.array(losses)).max(), np.abs(p_cpu - p_gpu).max()
    print(f"svgp training: loss {losses[0]:.6f} -> {losses[-1]:.6f}; |gpu - cpu| losses {d_loss:.2e} (bar {bar_loss:.2e}), "
          f"parameters {d_par:.2e} (bar {bar_par:.2e})")
    assert all(b < a for a, b in zip(losses, losses[1:])), "the losses do not decrease"
    assert d_loss <= bar_loss and d_par <= bar_par
    assert abs(model.noise - (T.softplus(cpu[4]) + 1e-4)) <= 1e-12 and abs(model.mean_constant - cpu[3]) <= bar_par


def test_full_batch_training_approaches_the_closed_form_optimum():
    """Full-batch gradient ascent with c and the noise frozen.  In m the ELBO is quadratic with curvature at most
    lambda_max(A A^T) / (N sigma^2) + 1 / N (10.2 here), so a step of 0.05 -- a quarter of 2 / 10.2 -- climbs monotonically;
    the ELBO can never pass the closed-form optimum.  The helper's CPU loop on this problem closes 97.3 % of the initial
    gap in 300 epochs (the flat directions of curvature 1 / N carry the rest); the library must close 90 %."""
    import projected_langevin_sampling_amd as pkg

    n, m, lr, epochs = 200, 17, 0.05, 300
    x, y = _data(n, 2, 42)
    z = x[:m].clone()
    kernel = pkg.ARDKernel([0.6, 0.8], 1.2)
    model = pkg.SVGP(kernel, z, noise=0.05, mean_init_std=0.0).fit_data(x, y)
    st = model._dev
    At = st["At"].cpu().contiguous()
    rho = float(model.scalars[1])
    curvature = torch.linalg.eigvalsh(At.T @ At).max().item() / (n * model.noise) + 1.0 / n
    assert lr * curvature < 1.0
    m_star, l_star = T.closed_form_optimum(At, y, 0.0, rho)
    best = T.evaluate(At.numpy(), st["q"].cpu().numpy(), y.numpy(), m_star.numpy(), l_star.numpy(), 0.0, rho, None, n)[0]
    ident = torch.arange(n)
    elbos = [-model.sgd_epoch(ident, n, lr, train_mean=False, train_noise=False).item() for _ in range(epochs)]
    print(f"full batch: ELBO {elbos[0]:.6f} -> {elbos[-1]:.6f}, optimum {best:.6f}, "
          f"gap left {(best - elbos[-1]) / (best - elbos[0]):.4f}")
    assert float(model.scalars[1]) == rho and model.mean_constant == 0.0, "a frozen scalar moved"
    assert all(e <= best for e in elbos), "an ELBO above the optimum"
    assert all(b >= a for a, b in zip(elbos, elbos[1:])), "the ELBO does not climb"
    assert best - elbos[-1] < 0.1 * (best - elbos[0])


def test_predict_and_temper_against_the_helper():
    import projected_langevin_sampling_amd as pkg

    n, m, t = 130, 17, 40
    x, y = _data(n, 2, 43)
    xt, yt = _data(t, 2, 44)
    z = x[:m].clone()
    ls, s, jitter = torch.tensor([0.6, 0.8], dtype=F64), 1.2, 1e-6
    model = pkg.SVGP(pkg.ARDKernel(ls, s), z, noise=0.07, mean_constant=0.1).fit_data(x, y)
    inp = T.make_inputs(44, n, m)
    model.variational_mean.copy_(inp["mean"])
    model.chol_variational_covar.copy_(torch.tril(inp["Ls"]))

    def k(a, b):
        return s * torch.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) / ls).square().sum(-1))

    kzz = k(z, z) + jitter * torch.eye(m, dtype=F64)
    assert torch.linalg.cond(kzz).item() <= 1e6
    low = torch.linalg.cholesky(kzz)
    a = torch.linalg.solve_triangular(low, k(z, xt), upper=False)  # (M, t)
    want_mean = 0.1 + a.T @ inp["mean"]
    want_var = s + jitter - a.square().sum(dim=0) + (a.T @ torch.tril(inp["Ls"])).square().sum(dim=1)
    mean, var, obs = (v.cpu() for v in model.predict(xt))
    e_mean = ((mean - want_mean).abs().max() / s).item()
    e_var = ((var - want_var).abs().max() / s).item()
    e_obs = ((obs - (want_var + model.noise)).abs().max() / s).item()
    print(f"svgp predict: mean {e_mean:.2e}, latent variance {e_var:.2e}, observation variance {e_obs:.2e} (relative to s)")
    assert abs(model.noise - 0.07) <= 1e-15
    assert e_mean <= 1e-11 and e_var <= 1e-10 and e_obs <= 1e-10
    # TemperGP on the SVGP and on an ExactGP: the scale formula of TemperPLS on the observation variance
    exact = pkg.ExactGP(x, y, "rbf")
    for gp in (model, exact):
        mean_c, _, obs_c = (v.cpu() for v in gp.predict(xt))
        temper = pkg.TemperGP(gp, xt, yt)
        want = 2 * torch.mean((yt - mean_c).square() / obs_c).item()
        assert abs(temper.scale - want) <= 1e-12 * abs(want)
        m2, lat2, obs2 = temper(xt)
        m1, lat1, obs1 = gp.predict(xt)
        assert torch.equal(m2, m1) and torch.equal(lat2, lat1 * temper.scale) and torch.equal(obs2, obs1 * temper.scale)
    with pytest.raises(TypeError, match="ExactGP or an SVGP"):
        pkg.TemperGP(object(), xt, yt)


def test_end_to_end_on_the_library_alone():
    """exact_gp_runner -> averaged kernel and noise -> inducing points -> PLSKernel -> train_svgp_runner"""
    import projected_langevin_sampling_amd as pkg

    x, y = _data(400, 2, 45)
    models = pkg.exact_gp_runner(x, y, "rbf", subsample_size=150, seed=5, number_of_epochs=5, learning_rate=0.05,
                                 number_of_iterations=2, early_stopper_patience=10.0)
    kernel = pkg.construct_average_ard_kernel(models)
    noise = pkg.construct_average_gaussian_noise(models)
    z = x[:20].clone()
    pls_kernel = pkg.PLSKernel(kernel, z)
    model, losses, best = pkg.train_svgp_runner(x, y, z, pls_kernel, seed=6, number_of_epochs=5, batch_size=128,
                                                learning_rate_upper=1e-1, learning_rate_lower=1e-3,
                                                number_of_learning_rate_searches=3, early_stopper_patience=1e9,
                                                observation_noise=noise)
    assert model is not None and len(losses) == 5 and np.isfinite(losses).all()
    lasts = {}
    for lr in np.logspace(-3, -1, 3):
        _, each = pkg.train_svgp(x, y, z, pls_kernel, 6, 5, 128, float(lr), 1e9, likelihood_noise=noise)
        lasts[float(lr)] = each[-1]
    assert best == min(lasts, key=lasts.get) and losses[-1] == lasts[best]
    mean, var, obs = model.predict(x[:50])
    assert torch.isfinite(mean).all() and (var > 0).all() and (obs > var).all()


def test_what_is_rejected_and_what_returns_none():
    import projected_langevin_sampling_amd as pkg

    x, y = _data(300, 2, 46)
    kernel = pkg.ARDKernel([0.6, 0.8], 1.2)
    with pytest.raises(ValueError, match="257 inducing points"):
        pkg.SVGP(kernel, x[:257])
    inp = T.make_inputs(47, 300, 8, 40)
    dev = Dev(inp)
    dev.desc.m = 257
    with pytest.raises(pkg._lib.PlsHipError, match="257 inducing points > 256"):
        dev.evaluate()
    # a zero on L_s's diagonal: log 0 in the KL term, a non-finite loss, (None, None) rather than an exception
    inp["Ls"][3, 3] = 0.0
    out = Dev(inp).evaluate()[0].cpu()
    assert not np.isfinite(out[0].item()) and not np.isfinite(out[4].item())
    model = pkg.SVGP(kernel, x[:8]).fit_data(x, y)
    model.chol_variational_covar[3, 3] = 0.0
    assert not np.isfinite(model.sgd_epoch(torch.arange(300), 100, 0.01).item())
    import projected_langevin_sampling_amd.gaussian_process as G

    class ZeroDiagonal(G.SVGP):
        def fit_data(self, x, y):
            super().fit_data(x, y)
            self.chol_variational_covar[0, 0] = 0.0
            return self

    original = G.SVGP
    G.SVGP = ZeroDiagonal
    try:
        assert pkg.train_svgp(x, y, x[:8], kernel, 0, 3, 100, 0.01, 1e9) == (None, None)
    finally:
        G.SVGP = original
