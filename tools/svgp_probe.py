"""What one SVGP minibatch step and one epoch cost through pls_svgp_sgd_epoch, beside the same formulas through torch
autograd in fp64 on the same card in the same run (tests/svgp_truth.py's differentiable ELBO moved to the device: the
reference's route without gpytorch's overhead).

    python tools/svgp_probe.py [--out profiles/svgp.txt] [--repeats 5]
    python tools/svgp_probe.py --likelihood all [--parent-library OTHER/libplship.so] [--out profiles/svgp_quadrature.txt]

``--likelihood gaussian`` (the default) writes the table of profiles/svgp.txt.  ``bernoulli`` / ``student_t`` / ``all`` time the
minibatch step of the quadrature likelihoods through pls_svgp_lik_sgd_epoch beside the Gaussian step of this library, the
Gaussian step of another build of the library (``--parent-library``: the parent commit's, same run, same inputs) and torch
autograd of tests/svgp_quadrature_truth.py's ELBO, each with the spread (min .. max) of its repeats.

Shapes (N, M, B): (1000, 32, 100); (1000, 100, 1000) full batch with the noise frozen -- the reference profiler's shape
(experiments/profiler/main.py:85-123); (36000, 191, 5000) -- the largest of the reference's drivers.  Per shape: an epoch
(all minibatch steps + the full-data loss) between two device events, median of the repeats after a warm-up epoch; the
full-data loss alone; microseconds per step = (epoch - loss) / steps.  Both columns run the same index batches from the
same starting state, and the states they reach are compared.  Needs the MI355X; there is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import projected_langevin_sampling_amd as pkg  # noqa: E402
import svgp_quadrature_truth as QT  # noqa: E402
import svgp_truth as T  # noqa: E402

F64 = torch.float64
SHAPES = [(1000, 32, 100, True), (1000, 100, 1000, False), (36000, 191, 5000, True)]  # N, M, B, train the noise
LR = 1e-3


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    timed.spread = (min(ms), max(ms))
    return statistics.median(ms)


class Library:
    """``lik``: (code, nu); a quadrature likelihood goes through the pls_svgp_lik_* entries.  ``path``: another build of the
    library (its Gaussian entries only)."""

    def __init__(self, inp, batch, train_noise, lik=(QT.GAUSSIAN, 0.0), path=None):
        import ctypes

        self.L = L = pkg._lib
        self.lib = L.load()
        if path:
            self.lib = ctypes.CDLL(path)
            for name in ("pls_svgp_workspace_bytes", "pls_svgp_elbo_grad", "pls_svgp_sgd_epoch"):
                getattr(self.lib, name).restype, getattr(self.lib, name).argtypes = L.SIGNATURES[name]
        self.n, self.m = inp["At"].shape
        self.at, self.q, self.y = inp["At"].cuda().contiguous(), inp["q"].cuda(), inp["y"].cuda()
        self.lik = lik
        self.lik_desc = L.SvgpLikDesc()
        self.lik_desc.deg_free = lik[1]
        self.desc = self.lik_desc.base
        self.desc.At, self.desc.ldat, self.desc.q, self.desc.y = self.at.data_ptr(), self.m, self.q.data_ptr(), self.y.data_ptr()
        self.desc.n, self.desc.m, self.desc.likelihood = self.n, self.m, lik[0]
        quadrature = lik[0] != QT.GAUSSIAN
        self.ref = ctypes.byref(self.lik_desc) if quadrature else ctypes.byref(self.desc)
        self.fn_epoch = self.lib.pls_svgp_lik_sgd_epoch if quadrature else self.lib.pls_svgp_sgd_epoch
        self.fn_value = self.lib.pls_svgp_lik_elbo_grad if quadrature else self.lib.pls_svgp_elbo_grad
        self.start = (inp["mean"].cuda(), torch.tril(inp["Ls"]).cuda().contiguous(), torch.tensor([inp["c"], inp["rho"]], dtype=F64).cuda())
        self.batch, self.flags = batch, L.SVGP_TRAIN_MEAN | (L.SVGP_TRAIN_NOISE if train_noise else 0)
        self.bytes = self.lib.pls_svgp_workspace_bytes(self.n, self.m, batch)
        self.ws = torch.empty(self.bytes // 8, dtype=F64, device="cuda")
        self.loss = torch.empty(5, dtype=F64, device="cuda")
        self.reset()

    def reset(self):
        self.mean, self.ls, self.scalars = (t.clone() for t in self.start)

    def epoch(self, perm):
        L = self.L
        L.check(self.fn_epoch(self.ref, self.mean.data_ptr(), self.ls.data_ptr(), self.m, self.scalars.data_ptr(), perm.data_ptr(),
                              self.batch, LR, self.flags, self.loss.data_ptr(), self.ws.data_ptr(), self.bytes, L.stream_ptr()),
                "pls_svgp_sgd_epoch")

    def value(self):
        L = self.L
        L.check(self.fn_value(self.ref, self.mean.data_ptr(), self.ls.data_ptr(), self.m, self.scalars.data_ptr(), None, self.n,
                              self.loss.data_ptr(), None, None, self.m, self.ws.data_ptr(), self.bytes, L.stream_ptr()),
                "pls_svgp_elbo_grad")


class Autograd:
    def __init__(self, lib: Library, train_noise):
        self.lib, self.train_noise = lib, train_noise and lib.lik[0] != QT.BERNOULLI
        self.reset()

    def reset(self):
        mean, ls, scalars = self.lib.start
        self.mean, self.ls = mean.clone().requires_grad_(True), ls.clone().requires_grad_(True)
        self.c, self.rho = scalars[0].clone().requires_grad_(True), scalars[1].clone().requires_grad_(self.train_noise)
        self.params = [self.mean, self.ls, self.c] + ([self.rho] if self.train_noise else [])

    def elbo(self, idx):
        if self.lib.lik[0] != QT.GAUSSIAN:
            return QT.elbo_torch(*self.lib.lik, self.lib.at, self.lib.q, self.lib.y, self.mean, self.ls, self.c, self.rho, idx,
                                 self.lib.n)
        return T.elbo_torch(self.lib.at, self.lib.q, self.lib.y, self.mean, self.ls, self.c, self.rho, idx, self.lib.n)

    def epoch(self, perm):
        for first in range(0, self.lib.n, self.lib.batch):
            for p in self.params:
                p.grad = None
            (-self.elbo(perm[first:first + self.lib.batch])).backward()
            with torch.no_grad():
                for p in self.params:
                    p.sub_(LR * p.grad)
        with torch.no_grad():
            self.loss = -self.elbo(None)

    def value(self):
        with torch.no_grad():
            self.loss = -self.elbo(None)


def agreement(lib, auto):
    pairs = [(lib.mean, auto.mean.detach()), (lib.ls, torch.tril(auto.ls.detach())),
             (lib.scalars, torch.stack([auto.c.detach(), auto.rho.detach()])), (lib.loss[:1], auto.loss.reshape(1))]
    return max(((x - y).abs().max() / y.abs().max()).item() for x, y in pairs)


def quadrature_table(args):
    """the minibatch step of every likelihood asked for, beside the Gaussian step of this build and of --parent-library"""
    names = {"bernoulli": [("bernoulli", (QT.BERNOULLI, 0.0))], "student_t": [("student_t nu=4.5", (QT.STUDENT_T, 4.5))]}
    names["all"] = names["bernoulli"] + names["student_t"]
    rows = [("gaussian", (QT.GAUSSIAN, 0.0), None)]
    if args.parent_library:
        rows.append(("gaussian, parent", (QT.GAUSSIAN, 0.0), args.parent_library))
    rows += [(name, lik, None) for name, lik in names[args.likelihood]]
    lines = [f"# tools/svgp_probe.py --likelihood {args.likelihood} on {torch.cuda.get_device_name(0)}: the SVGP minibatch step, plain SGD",
             f"# (device events around a whole epoch, median of {args.repeats} after a warm-up epoch, min .. max of the repeats beside it);",
             "# step = (epoch - full-data loss) / steps.  lib = pls_svgp_sgd_epoch (gaussian) / pls_svgp_lik_sgd_epoch; 'gaussian, parent' = the",
             "# parent commit's build of the library in the same run; torch = the same ELBO (20-node quadrature) through torch autograd, fp64",
             "# agree = largest difference of m, tril L_s, c, rho, loss after one epoch from the same start, relative to the largest entry",
             f"{'N':>6s} {'M':>4s} {'B':>5s} {'steps':>5s} {'likelihood':>17s} | {'lib us/step':>11s} {'lib ms/epoch':>12s} {'min .. max':>17s} | "
             f"{'torch us/step':>13s} {'torch ms/epoch':>14s} {'min .. max':>17s} | {'torch/lib':>9s} {'agree':>8s}"]
    for n, m, b, train_noise in SHAPES:
        base = T.make_inputs(900000 + m, n, m)
        base["At"] = base["At"] / m**0.5
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
        steps = -(-n // b)
        for name, lik, path in rows:
            inp = dict(base, y=(base["y"] > 0).double()) if lik[0] == QT.BERNOULLI else base
            lib = Library(inp, b, train_noise, lik, path)
            lib.epoch(perm)
            epoch = timed(lambda: lib.epoch(perm), args.repeats)
            spread = timed.spread
            value = timed(lib.value, args.repeats)
            left = f"{n:6d} {m:4d} {b:5d} {steps:5d} {name:>17s} | {1e3 * (epoch - value) / steps:11.1f} {epoch:12.3f} {spread[0]:8.3f}{spread[1]:9.3f} | "
            if lik[0] == QT.GAUSSIAN:
                lines.append(left + f"{'':13s} {'':14s} {'':17s} | {'':9s} {'':8s}")
            else:
                auto = Autograd(lib, train_noise)
                lib.reset()
                lib.epoch(perm)
                auto.epoch(perm)
                torch.cuda.synchronize()
                agree = agreement(lib, auto)
                auto.reset()
                t_epoch = timed(lambda: auto.epoch(perm), args.repeats)
                t_spread = timed.spread
                t_value = timed(auto.value, args.repeats)
                lines.append(left + f"{1e3 * (t_epoch - t_value) / steps:13.1f} {t_epoch:14.3f} {t_spread[0]:8.3f}{t_spread[1]:9.3f} | "
                                    f"{t_epoch / epoch:9.2f} {agree:8.1e}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--likelihood", default="gaussian", choices=["gaussian", "bernoulli", "student_t", "all"])
    ap.add_argument("--parent-library", default=None, help="another build of libplship.so whose Gaussian step is timed beside this one")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    if args.likelihood != "gaussian":
        args.out = args.out or os.path.join(ROOT, "profiles", "svgp_quadrature.txt")
        lines = quadrature_table(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "svgp.txt")
    lines = [f"# tools/svgp_probe.py on {torch.cuda.get_device_name(0)}: SVGP (fixed kernel, Gaussian likelihood), plain SGD",
             f"# (device events around a whole epoch, median of {args.repeats} after a warm-up epoch); step = (epoch - loss) / steps",
             "# lib = pls_svgp_sgd_epoch (one call per epoch); torch = the same ELBO through torch autograd, fp64, same card, same run",
             "# agree = largest difference of m, tril L_s, c, rho after one epoch from the same start, relative to the largest entry",
             f"{'N':>6s} {'M':>4s} {'B':>5s} {'steps':>5s} {'noise':>6s} | {'lib us/step':>11s} {'lib loss ms':>11s} {'lib ms/epoch':>12s} | "
             f"{'torch us/step':>13s} {'torch loss ms':>13s} {'torch ms/epoch':>14s} | {'torch/lib epoch':>15s} {'agree':>8s}"]
    for n, m, b, train_noise in SHAPES:
        inp = T.make_inputs(900000 + m, n, m)
        inp["At"] = inp["At"] / m**0.5  # (rows of unit scale whatever M is)
        lib = Library(inp, b, train_noise)
        auto = Autograd(lib, train_noise)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
        steps = -(-n // b)
        # one epoch each from the same start: the states must agree
        lib.epoch(perm)
        auto.epoch(perm)
        torch.cuda.synchronize()
        agree = agreement(lib, auto)
        res = {}
        for name, side in (("lib", lib), ("torch", auto)):
            side.reset()
            epoch = timed(lambda: side.epoch(perm), args.repeats)
            value = timed(side.value, args.repeats)
            res[name] = (1e3 * (epoch - value) / steps, value, epoch)
        lines.append(f"{n:6d} {m:4d} {b:5d} {steps:5d} {'learnt' if train_noise else 'frozen':>6s} | {res['lib'][0]:11.1f} {res['lib'][1]:11.3f} "
                     f"{res['lib'][2]:12.3f} | {res['torch'][0]:13.1f} {res['torch'][1]:13.3f} {res['torch'][2]:14.3f} | "
                     f"{res['torch'][2] / res['lib'][2]:15.2f} {agree:8.1e}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
