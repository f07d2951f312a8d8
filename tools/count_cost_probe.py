#!/usr/bin/env python3
"""Times one train_pls iteration with a negative-binomial cost under the exponential link at the three `reference_scale`
shapes of bench.py, (N, M, J) = (100, 10, 64), (1000, 32, 100), (4096, 128, 512), on both bases.

    python tools/count_cost_probe.py --variant native|unfused|bernoulli [--root TREE] [--iterations 200] [--repeats 7]

  native     NegativeBinomialCost / ExponentialLinkFunction: the library's fused routes
  unfused    the only way a build without the cost offers it: a torch PLSCost subclass, which train_pls runs through
             pls_onb_forward / pls_ipb_forward -> torch code -> the particle update.  Needs nothing of the new cost, so
             --root may point at a checkout (and build) of the commit before it
  bernoulli  Bernoulli/sigmoid on the same problem, for information: the pair whose routes the new one shares

One JSON line per (shape, basis): microseconds per iteration (step + energy + early-stop test), the median, minimum and
maximum over --repeats runs of --iterations iterations, each run ended by a device synchronise; 30 warm-up iterations per
case.  Compare variants from processes started in turn in one session (the host is shared: see the spread)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

SHAPES = ((100, 10, 64, 1), (1000, 32, 100, 1), (4096, 128, 512, 4))
DISPERSION = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("native", "unfused", "bernoulli"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd import costs, link_functions
    from projected_langevin_sampling_amd.basis import InducingPointBasis, OrthonormalBasis
    from projected_langevin_sampling_amd.trainers import train_pls

    assert torch.cuda.is_available(), "count_cost_probe needs the GPU: there is no CPU timing"
    print(f"count_cost_probe: package from {os.path.dirname(pkg.__file__)}", file=sys.stderr)
    torch.set_default_dtype(torch.float64)

    class TorchNegativeBinomial(costs.PLSCost):
        """what a user writes in torch where the library has no such cost"""

        def __init__(self, y_train, dispersion):
            class Exp(link_functions.PLSLinkFunction):
                def transform(self, y):
                    return torch.exp(y)

            super().__init__(link_function=Exp(), observation_noise=None)
            self.y_train, self.r = y_train, float(dispersion)
            self._y = y_train.cuda()[:, None]
            self._lr = torch.log(torch.tensor(self.r)).item()

        def predict(self, prediction_samples):
            raise NotImplementedError

        def calculate_cost(self, untransformed_train_prediction_samples):
            t = untransformed_train_prediction_samples - self._lr
            return (self.r * torch.nn.functional.softplus(t, threshold=700.0) + self._y * torch.nn.functional.softplus(-t, threshold=700.0)).sum(dim=0)

        def calculate_cost_derivative(self, untransformed_train_prediction_samples, force_autograd=False):
            t = untransformed_train_prediction_samples - self._lr
            return self.r * torch.sigmoid(t) - self._y * torch.sigmoid(-t)

    for n, m, j, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(n, d, generator=g) * 2 - 1
        z = x[torch.randperm(n, generator=g)[:m]].clone()
        fstar = torch.sin(2.0 * x.sum(dim=1))
        y = torch.poisson(torch.exp(1.0 + fstar), generator=g)
        kern = pkg.PLSKernel(pkg.ARDKernel(torch.full((d,), 0.5), 1.0), z)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bases = (("orthonormal", OrthonormalBasis(kern, z, x, 1e-8, verbose=False)), ("inducing_point", InducingPointBasis(kern, z, y[:m], x)))
        for bname, basis in bases:
            if args.variant == "native":
                cost = costs.NegativeBinomialCost(y, link_functions.ExponentialLinkFunction(), DISPERSION)
                assert cost.is_native()
            elif args.variant == "unfused":
                cost = TorchNegativeBinomial(y, DISPERSION)
                assert not cost.is_native()
            else:
                cost = costs.BernoulliCost((y > 2).double(), link_functions.SigmoidLinkFunction())
            pls = pkg.PLS(basis, cost)
            u = (0.1 * torch.randn(basis.approximation_dimension, j, generator=g)).cuda()
            eta = 1e-13  # (timing only, as bench.py's block: inside every stability bound, so no run stops early)
            train_pls(pls, u.clone(), 30, eta, 1e9)
            runs = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, e = train_pls(pls, u.clone(), args.iterations, eta, 1e9)
                torch.cuda.synchronize()
                assert len(e) == args.iterations
                runs.append((time.perf_counter() - t0) / args.iterations * 1e6)
            print(json.dumps({"label": args.label, "variant": args.variant, "n": n, "m": m, "j": j, "basis": bname,
                              "us_per_iteration": {"median": round(statistics.median(runs), 2), "min": round(min(runs), 2),
                                                   "max": round(max(runs), 2)},
                              "iterations": args.iterations, "repeats": args.repeats}), flush=True)


if __name__ == "__main__":
    main()
