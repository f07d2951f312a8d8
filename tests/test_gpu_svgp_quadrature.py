"""GPU: the SVGP entries with a quadrature likelihood (csrc/svgp.hip, pls_svgp_lik_*) -- every output of
pls_svgp_lik_elbo_grad for the Bernoulli and the Student-t likelihood against the 50-digit fixture and the fsum helper
within (M + B + 16 + c) eps S (S and c: tests/svgp_quadrature_truth.py; c comes from the CPU helper and the fixture), the
bit-for-bit equalities the header promises (the Gaussian likelihood through the new entries = the old entries among
them), pls_svgp_lik_sgd_epoch against its replay, train_svgp(likelihood=...) against the helper's CPU loop, prediction,
TemperGP and the classification chain on the library alone.

Shapes: as tests/test_gpu_svgp.py (tiles of 32 points and 16 inducing points, rounds of 64 columns); the quadrature deals
a wave's 8 points over 8 lanes each, so B = 1, 2, 31 ... 33, 63, 65 leave groups and whole waves without a point."""
import ctypes

import numpy as np
import pytest
import torch

import svgp_quadrature_truth as QT
import svgp_truth as T

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
LIKS = sorted(QT.LIKELIHOODS)


class Dev:
    """the inputs of svgp_truth.make_inputs on the device behind a pls_svgp_lik_desc, every buffer padded with NaN: the
    padding columns of At, the upper triangle and the padding of L_s, and a tail behind every output.  ``lik``: a name of
    svgp_quadrature_truth.LIKELIHOODS or "gaussian"; the inputs already hold that likelihood's targets."""

    TAIL = 3

    def __init__(self, inp, lik, ls_offset=0):
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
        self.code, self.nu = (0, 0.0) if lik == "gaussian" else QT.LIKELIHOODS[lik]
        self.desc = L.SvgpLikDesc()
        base = self.desc.base
        base.At, base.ldat, base.q, base.y = self.at.data_ptr(), self.ldat, self.q.data_ptr(), self.y.data_ptr()
        base.n, base.m, base.likelihood = n, m, self.code
        self.desc.deg_free = self.nu
        self.tril = (torch.from_numpy(k).cuda(), torch.from_numpy(l).cuda())
        nbytes = self.lib.pls_svgp_workspace_bytes(n, m, n)
        self.ws = torch.full((nbytes // 8 + 2,), NAN, dtype=F64, device="cuda")
        self.ws_bytes = nbytes

    def evaluate(self, idx="case", gradients=True, old_entry=False, expect=0):
        """one pls_svgp_lik_elbo_grad call (``old_entry``: pls_svgp_elbo_grad on the base descriptor) ->
        (out (5), grad_m (M), grad_L (M, M+1 with its padding)); sentinels checked.  ``expect``: the status the call must
        return; a rejected call must leave every output as it was."""
        m, L = self.m, self.L
        if isinstance(idx, str):
            idx = self.inp["idx"]
        b = self.n if idx is None else idx.numel()
        idx_dev = None if idx is None else idx.cuda()
        out = torch.full((5 + self.TAIL,), NAN, dtype=F64, device="cuda")
        gm = torch.full((m + self.TAIL,), NAN, dtype=F64, device="cuda")
        gl = torch.full((m, m + 1), NAN, dtype=F64, device="cuda")
        before = self.ls_buf.clone()
        fn = self.lib.pls_svgp_elbo_grad if old_entry else self.lib.pls_svgp_lik_elbo_grad
        desc = ctypes.byref(self.desc.base) if old_entry else ctypes.byref(self.desc)
        rc = fn(desc, self.mean.data_ptr(), self.ls.data_ptr(), self.ldls, self.scalars.data_ptr(), L.ptr(idx_dev), b,
                out.data_ptr(), gm.data_ptr() if gradients else None, gl.data_ptr() if gradients else None, m + 1,
                self.ws.data_ptr(), self.ws_bytes, L.stream_ptr())
        torch.cuda.synchronize()
        if expect:
            assert rc == expect, (rc, self.lib.pls_last_error())
            assert torch.isnan(out).all() and torch.isnan(gm).all() and torch.isnan(gl).all() and torch.isnan(self.ws).all()
            return self.lib.pls_last_error()
        L.check(rc, "pls_svgp_lik_elbo_grad")
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


def _check(name, lik, got, want_hi, want_lo, scale, m, b):
    err = T.relative_error(got, want_hi, want_lo, scale)
    worst = int(np.argmax(err))
    helper, c = QT.epilogue_allowance()
    print(f"{lik} {name}: worst |device - truth| / S = {err.max() / T.EPS:.2f} eps at output {worst} "
          f"(bar {QT.bar(m, b) / T.EPS:.0f} eps; helper {helper:.2f} eps, c = {c:.0f})")
    assert np.isfinite(got).all()
    if QT.LIKELIHOODS[lik][0] == QT.BERNOULLI:
        assert got[2] == 0.0 and not np.signbit(got[2])
    assert (err <= QT.bar(m, b)).all()


@pytest.mark.parametrize("name", sorted(QT.CASES))
@pytest.mark.parametrize("lik", LIKS)
def test_every_output_against_the_50_digit_truth(lik, name):
    inp, _, scale = QT.cpu_case(lik, name)
    m, b, _ = QT.CASES[name]
    hi, lo = QT.truth(lik, name)
    dev = Dev(inp, lik)
    _check(name, lik, dev.vector(*dev.evaluate()), hi, lo, scale, m, b)


LARGER = [(15, 31), (16, 32), (17, 33), (64, 2), (65, 1), (130, 33), (191, 130), (256, 65)]
_larger_cache = {}


def _larger(lik, m, b, evaluate=True):
    key = (lik, m, b)
    if key not in _larger_cache:
        inp = T.make_inputs(810000 + 1000 * m + b, 300, m, b)
        inp = inp if lik == "gaussian" else QT.with_targets(lik, inp)
        if evaluate:
            _larger_cache[key] = (inp, QT.evaluate_inputs(lik, inp), QT.evaluate_inputs(lik, inp, scale=True))
        else:
            return inp, None, None
    return _larger_cache[key]


@pytest.mark.parametrize("m,b", LARGER)
@pytest.mark.parametrize("lik", LIKS)
def test_every_output_against_the_fsum_helper(lik, m, b):
    inp, want, scale = _larger(lik, m, b)
    dev = Dev(inp, lik)
    _check(f"m{m}-b{b}", lik, dev.vector(*dev.evaluate()), want, np.zeros_like(want), scale, m, b)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("m,b", [(17, 65), (65, 33), (191, 130)])
@pytest.mark.parametrize("lik", ["bernoulli", "student4.5", "gaussian"])
def test_bit_for_bit_equalities(lik, m, b):
    inp = _larger(lik, m, b, evaluate=False)[0] if (m, b) in LARGER else T.make_inputs(820000 + m, 300, m, b)
    inp = inp if lik == "gaussian" else QT.with_targets(lik, inp)
    dev = Dev(inp, lik)

    def same(r1, r2):
        k, l = dev.tril
        return all(torch.equal(_bits(x), _bits(y)) for x, y in ((r1[0], r2[0]), (r1[1], r2[1]), (r1[2][k, l], r2[2][k, l])))

    first = dev.evaluate()
    assert torch.isfinite(first[0]).all()
    assert same(first, dev.evaluate()), "two calls differ"
    ident = torch.arange(b, dtype=torch.int64)
    head = dict(inp, At=inp["At"][:b], q=inp["q"][:b], y=inp["y"][:b], n=b)
    part = Dev(head, lik).evaluate(idx=ident)
    assert same(Dev(head, lik).evaluate(idx=None), part), "NULL idx and the identity list differ"
    assert torch.equal(_bits(dev.evaluate(idx=ident)[0][3:5]), _bits(part[0][3:5]))
    assert torch.equal(_bits(dev.evaluate(gradients=False)[0]), _bits(first[0])), "the value-only kernel differs"
    assert same(first, Dev(inp, lik, ls_offset=1).evaluate()), "L_s at an odd 8-byte offset differs"
    if lik == "gaussian":
        assert same(first, dev.evaluate(old_entry=True)), "the Gaussian likelihood through pls_svgp_lik_elbo_grad differs"
        assert torch.equal(_bits(dev.evaluate(gradients=False, old_entry=True)[0]), _bits(first[0]))


def _epoch(dev, perm_dev, batch_size, lr, flags, old_entry=False):
    L = dev.L
    loss = torch.full((1 + Dev.TAIL,), NAN, dtype=F64, device="cuda")
    fn = dev.lib.pls_svgp_sgd_epoch if old_entry else dev.lib.pls_svgp_lik_sgd_epoch
    desc = ctypes.byref(dev.desc.base) if old_entry else ctypes.byref(dev.desc)
    L.check(fn(desc, dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls, dev.scalars.data_ptr(), perm_dev.data_ptr(), batch_size,
               lr, flags, loss.data_ptr(), dev.ws.data_ptr(), dev.ws_bytes, L.stream_ptr()), "pls_svgp_lik_sgd_epoch")
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all()
    return loss


EPOCHS = ([("student3", f) for f in range(4)] + [("bernoulli", 1), ("bernoulli", 3)])


@pytest.mark.parametrize("n,m,batch_size", [(150, 17, 64), (100, 65, 33)])
@pytest.mark.parametrize("lik,flags", EPOCHS)
def test_the_epoch_equals_its_replay(lik, flags, n, m, batch_size):
    """pls_svgp_lik_sgd_epoch over a shuffled perm (ragged last batch) = pls_svgp_lik_elbo_grad per batch + p - lr * (-g)
    by torch, bit for bit in m, tril L_s, c and rho; a frozen scalar keeps its bits, and a Bernoulli likelihood never
    moves rho; loss_out = - the value-only ELBO on all rows"""
    lr = 0.05
    inp = QT.with_targets(lik, T.make_inputs(830000 + m, n, m))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n + m))
    dev, rep = Dev(inp, lik), Dev(inp, lik)
    L = dev.L
    loss = _epoch(dev, perm.cuda(), batch_size, lr, flags)
    k, l = rep.tril
    for first in range(0, n, batch_size):
        out, gm, gl = rep.evaluate(idx=perm[first:first + batch_size])
        rep.mean.copy_(rep.mean - lr * (-gm))
        rep.ls[k, l] = rep.ls[k, l] - lr * (-gl[k, l])
        if flags & L.SVGP_TRAIN_MEAN:
            rep.scalars[0] = rep.scalars[0] - lr * (-out[1])
        if flags & L.SVGP_TRAIN_NOISE and dev.code != QT.BERNOULLI:
            rep.scalars[1] = rep.scalars[1] - lr * (-out[2])
    assert torch.equal(_bits(dev.mean), _bits(rep.mean))
    assert torch.equal(_bits(dev.ls_buf), _bits(rep.ls_buf))  # (the NaN upper triangle and padding included)
    assert torch.equal(_bits(dev.scalars), _bits(rep.scalars))
    start = torch.tensor([inp["c"], inp["rho"]], dtype=F64)
    moved = _bits(dev.scalars.cpu()) != _bits(start)
    assert moved.tolist() == [bool(flags & 1), bool(flags & 2) and dev.code != QT.BERNOULLI]
    assert not torch.equal(_bits(dev.mean.cpu()), _bits(inp["mean"]))
    value = rep.evaluate(idx=None, gradients=False)[0]
    assert torch.isfinite(loss[0])
    assert torch.equal(_bits(loss[:1]), _bits(-value[:1]))
    assert torch.isnan(dev.ws[dev.ws_bytes // 8:]).all()


def test_the_gaussian_epoch_and_prediction_through_the_new_entries_are_the_old_bits():
    n, m, batch_size, lr = 150, 17, 64, 0.05
    inp = T.make_inputs(830000 + m, n, m)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n + m)).cuda()
    new, old = Dev(inp, "gaussian"), Dev(inp, "gaussian")
    l_new, l_old = _epoch(new, perm, batch_size, lr, 3), _epoch(old, perm, batch_size, lr, 3, old_entry=True)
    assert torch.equal(_bits(l_new[:1]), _bits(l_old[:1])) and torch.equal(_bits(new.mean), _bits(old.mean))
    assert torch.equal(_bits(new.ls_buf), _bits(old.ls_buf)) and torch.equal(_bits(new.scalars), _bits(old.scalars))
    assert not torch.equal(_bits(new.scalars.cpu()), _bits(torch.tensor([inp["c"], inp["rho"]], dtype=F64)))
    for lik in ("gaussian", "bernoulli", "student3"):
        dev = Dev(inp, lik)
        t = 70
        bufs = [torch.full((t + Dev.TAIL,), NAN, dtype=F64, device="cuda") for _ in range(5)]
        L = dev.L
        L.check(dev.lib.pls_svgp_predict(dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls, dev.scalars.data_ptr(), dev.at.data_ptr(),
                                         dev.ldat, dev.q.data_ptr(), t, m, bufs[0].data_ptr(), bufs[1].data_ptr(), L.stream_ptr()),
                "pls_svgp_predict")
        L.check(dev.lib.pls_svgp_lik_predict(ctypes.byref(dev.desc), dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls,
                                             dev.scalars.data_ptr(), dev.at.data_ptr(), dev.ldat, dev.q.data_ptr(), t, m,
                                             bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), L.stream_ptr()),
                "pls_svgp_lik_predict")
        torch.cuda.synchronize()
        assert all(torch.isnan(buf[t:]).all() and torch.isfinite(buf[:t]).all() for buf in bufs)
        assert torch.equal(_bits(bufs[0]), _bits(bufs[2])) and torch.equal(_bits(bufs[1]), _bits(bufs[3]))
        mean, var, obs = (buf[:t].cpu().numpy() for buf in bufs[2:])
        sig2 = QT.noise_of(dev.code, inp["rho"])
        if lik == "bernoulli":
            from scipy.special import ndtr

            want = ndtr(mean / np.sqrt(1.0 + var)) * ndtr(-mean / np.sqrt(1.0 + var))
        elif lik == "gaussian":
            want = var + sig2
        else:
            want = var + sig2 * dev.nu / (dev.nu - 2.0)
        assert (np.abs(obs - want) <= 1e-12 * np.abs(want)).all()
        # obs_out may be NULL
        L.check(dev.lib.pls_svgp_lik_predict(ctypes.byref(dev.desc), dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls,
                                             dev.scalars.data_ptr(), dev.at.data_ptr(), dev.ldat, dev.q.data_ptr(), t, m,
                                             bufs[2].data_ptr(), bufs[3].data_ptr(), None, L.stream_ptr()), "pls_svgp_lik_predict")
        torch.cuda.synchronize()
        assert torch.equal(_bits(bufs[0]), _bits(bufs[2])) and torch.equal(_bits(bufs[1]), _bits(bufs[3]))


def _data(n, d, seed, lik):
    """the regression data of tests/test_gpu_svgp.py; Bernoulli: labels sin(3 sum x) + 0.3 eps > 0; Student-t: one in ten
    targets shifted by +-3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g, dtype=F64) * 2 - 1
    eps = torch.randn(n, generator=g, dtype=F64)
    if lik == "bernoulli":
        return x, (torch.sin(3 * x.sum(dim=1)) + 0.3 * eps > 0).double()
    y = torch.sin(3 * x.sum(dim=1)) + 0.1 * eps
    if lik == "student":
        shift = torch.where(torch.arange(n) % 20 == 0, 3.0, -3.0).double()
        y = torch.where(torch.arange(n) % 10 == 0, y + shift, y)
    return x, y


@pytest.mark.parametrize("lik", ["bernoulli", "student"])
def test_training_follows_the_cpu_loop(lik):
    """train_svgp(likelihood=...) (one library call per epoch) against the helper's loop (autograd of the contract's
    formulas) on the same batches and the same whitened rows.  The bar comes from the CPU loop alone: rerun with every
    gradient component perturbed by a relative 1e-12 (alternating signs), 16 x the divergence of the losses and of the
    final parameters, floor 1e-11."""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.utils import set_seed

    n, m, bs, epochs, lr, seed = 300, 17, 65, 30, 0.02, 4
    x, y = _data(n, 2, 41, lik)
    z = x[:m].clone()
    kernel = pkg.PLSKernel(pkg.ARDKernel([0.6, 0.8], 1.2), z)
    likelihood = pkg.BernoulliLikelihood() if lik == "bernoulli" else pkg.StudentTLikelihood(4.5)
    code, nu = (QT.BERNOULLI, 0.0) if lik == "bernoulli" else (QT.STUDENT_T, 4.5)
    model, losses = pkg.train_svgp(x, y, z, kernel, seed, epochs, bs, lr, early_stopper_patience=1e9, likelihood=likelihood)
    assert model is not None and len(losses) == epochs
    set_seed(seed)
    mean0 = 1e-3 * torch.randn(m, dtype=F64)
    batches = [pkg.epoch_batches(n, bs) for _ in range(epochs)]
    assert [b.numel() for b in batches[0]] == [65, 65, 65, 65, 40]
    st = model._dev
    At, q = st["At"].cpu().contiguous(), st["q"].cpu()
    assert (q > 0).all()
    args = (code, nu, At, q, y, mean0, torch.eye(m, dtype=F64), 0.0, 0.0, batches, lr)
    cpu = QT.sgd_loop(*args)
    per = QT.sgd_loop(*args, perturb=1e-12)
    k, l = np.tril_indices(m)

    def params(mean, ls, c, rho):
        return np.concatenate([np.asarray(mean), np.asarray(ls)[k, l], [c, rho]])

    p_cpu, p_per = params(*cpu[1:]), params(*per[1:])
    p_gpu = params(model.variational_mean.cpu(), model.chol_variational_covar.cpu(), *model.scalars.cpu().tolist())
    bar_loss = max(16.0 * np.abs(np.array(cpu[0]) - np.array(per[0])).max(), 1e-11)
    bar_par = max(16.0 * np.abs(p_cpu - p_per).max(), 1e-11)
    d_loss, d_par = np.abs(np.array(cpu[0]) - np.array(losses)).max(), np.abs(p_cpu - p_gpu).max()
    print(f"svgp {lik} training: loss {losses[0]:.6f} -> {losses[-1]:.6f}; |gpu - cpu| losses {d_loss:.2e} (bar {bar_loss:.2e}), "
          f"parameters {d_par:.2e} (bar {bar_par:.2e})")
    assert all(b < a for a, b in zip(losses, losses[1:])), "the losses do not decrease"
    assert d_loss <= bar_loss and d_par <= bar_par
    if lik == "bernoulli":
        assert float(model.scalars[1]) == 0.0, "rho moved under a Bernoulli likelihood"
        with pytest.raises(AttributeError):
            model.noise
    else:
        assert abs(model.noise - T.softplus(cpu[4])) <= 1e-12 and cpu[4] != 0.0  # (no 1e-4 floor)


def test_predict_proba_student_variance_and_temper():
    import projected_langevin_sampling_amd as pkg
    from scipy.special import ndtr

    n, m, t = 130, 17, 40
    xt, yt = _data(t, 2, 44, "student")
    inp = T.make_inputs(44, n, m)
    for lik in ("bernoulli", "student"):
        x, y = _data(n, 2, 43, lik)
        z = x[:m].clone()
        likelihood = pkg.BernoulliLikelihood() if lik == "bernoulli" else pkg.StudentTLikelihood(3.0, noise=0.07)
        model = pkg.SVGP(pkg.ARDKernel([0.6, 0.8], 1.2), z, likelihood=likelihood, mean_constant=0.1).fit_data(x, y)
        plain = pkg.SVGP(pkg.ARDKernel([0.6, 0.8], 1.2), z, mean_constant=0.1).fit_data(x, y)
        for mod in (model, plain):
            mod.variational_mean.copy_(inp["mean"])
            mod.chol_variational_covar.copy_(torch.tril(inp["Ls"]))
        mean, var, obs = model.predict(xt)
        mean0, var0, _ = plain.predict(xt)
        assert torch.equal(_bits(mean), _bits(mean0)) and torch.equal(_bits(var), _bits(var0)), "not pls_svgp_predict's bits"
        mean, var, obs = mean.cpu().numpy(), var.cpu().numpy(), obs.cpu().numpy()
        if lik == "bernoulli":
            p = model.predict_proba(xt).cpu().numpy()
            want = ndtr(mean / np.sqrt(1.0 + var))
            print(f"predict_proba: worst |p - ndtr| = {np.abs(p - want).max():.2e}")
            assert np.abs(p - want).max() <= 1e-14 and (np.abs(obs - want * (1.0 - want)) <= 1e-14).all()
            with pytest.raises(TypeError, match="ExactGP or an SVGP"):
                pkg.TemperGP(object(), xt, yt)
        else:
            assert abs(model.noise - 0.07) <= 1e-15
            want = var + model.noise * 3.0 / (3.0 - 2.0)
            assert (np.abs(obs - want) <= 1e-12 * np.abs(want)).all()
            with pytest.raises(AttributeError, match="BernoulliLikelihood only"):
                model.predict_proba(xt)
            temper = pkg.TemperGP(model, xt, yt)
            scale = 2 * np.mean((yt.numpy() - mean) ** 2 / want)
            assert abs(temper.scale - scale) <= 1e-12 * abs(scale)
            m2, lat2, obs2 = temper(xt)
            m1, lat1, obs1 = model.predict(xt)
            assert torch.equal(m2, m1) and torch.equal(lat2, lat1 * temper.scale) and torch.equal(obs2, obs1 * temper.scale)


def test_end_to_end_classification_on_the_library_alone():
    """exact_gp_runner(likelihood="dirichlet") -> averaged kernel -> inducing points -> PLSKernel ->
    train_svgp_runner(likelihood=BernoulliLikelihood()).  Five epochs are short: the rates go up to 1 and a batch holds 40
    points (50 steps), because the CPU helper's loop on a stand-in for this problem (the same data, k(x, Z) k(Z, x') / M of an
    RBF kernel) leaves the latent function nearly flat -- every prediction on the majority's side -- after 20 steps at 0.1,
    and separates the classes at 1."""
    import projected_langevin_sampling_amd as pkg

    x, y = _data(400, 2, 45, "bernoulli")
    models = pkg.exact_gp_runner(x, y, "rbf", subsample_size=150, seed=5, number_of_epochs=5, learning_rate=0.05,
                                 number_of_iterations=2, early_stopper_patience=10.0, likelihood="dirichlet")
    kernel = pkg.construct_average_ard_kernel(models)
    z = x[:20].clone()
    pls_kernel = pkg.PLSKernel(kernel, z)
    rates = dict(learning_rate_upper=1.0, learning_rate_lower=1e-2, number_of_learning_rate_searches=3)
    model, losses, best = pkg.train_svgp_runner(x, y, z, pls_kernel, seed=6, number_of_epochs=5, batch_size=40,
                                                early_stopper_patience=1e9, likelihood=pkg.BernoulliLikelihood(), **rates)
    assert model is not None and len(losses) == 5 and np.isfinite(losses).all()
    lasts = {}
    for lr in np.logspace(-2, 0, 3):
        _, each = pkg.train_svgp(x, y, z, pls_kernel, 6, 5, 40, float(lr), 1e9, likelihood=pkg.BernoulliLikelihood())
        assert each is not None and np.isfinite(each).all()
        lasts[float(lr)] = each[-1]
    assert best == min(lasts, key=lasts.get) and losses[-1] == lasts[best]
    p = model.predict_proba(x).cpu()
    accuracy = ((p > 0.5).double() == y).double().mean().item()
    majority = max(y.mean().item(), 1.0 - y.mean().item())
    print(f"bernoulli svgp: training accuracy {accuracy:.3f}, majority class {majority:.3f}, best rate {best:g}")
    assert ((p > 0) & (p < 1)).all() and accuracy > majority


def test_what_is_rejected_and_what_returns_none():
    import projected_langevin_sampling_amd as pkg
    import projected_langevin_sampling_amd.gaussian_process as G

    inp = T.make_inputs(47, 300, 8, 40)
    dev = Dev(inp, "student3")
    dev.desc.base.likelihood = 3
    assert b"unknown likelihood" in dev.evaluate(expect=1)
    dev.desc.base.likelihood = QT.STUDENT_T
    for nu in (2.0, 0.5, float("nan")):
        dev.desc.deg_free = nu
        assert b"deg_free > 2" in dev.evaluate(expect=1)
    dev.desc.deg_free = 3.0
    dev.ws_bytes = 64
    assert b"needed" in dev.evaluate(expect=3)
    # v <= 0 at one point: its quadrature is not finite, and so is everything the point enters
    for lik in ("bernoulli", "student3"):
        bad = QT.with_targets(lik, T.make_inputs(47, 300, 8, 40))
        bad["q"][int(bad["idx"][5])] = -1e6
        out, gm, _ = Dev(bad, lik).evaluate()
        assert not np.isfinite(out[0].item()) and not torch.isfinite(gm).all()
    x, y = _data(300, 2, 46, "bernoulli")
    kernel = pkg.ARDKernel([0.6, 0.8], 1.2)

    class NegativeVariance(G.SVGP):
        def fit_data(self, x, y):
            super().fit_data(x, y)
            self._dev["q"][7] = -1e6
            return self

    original = G.SVGP
    G.SVGP = NegativeVariance
    try:
        assert pkg.train_svgp(x, y, x[:8], kernel, 0, 3, 100, 0.01, 1e9, likelihood=pkg.BernoulliLikelihood()) == (None, None)
    finally:
        G.SVGP = original
