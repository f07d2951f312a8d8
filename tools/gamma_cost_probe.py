#!/usr/bin/env python3
"""Times the Gamma cost (log link) beside its neighbours, in one process on one tree.

    python tools/gamma_cost_probe.py [--iterations 200] [--repeats 7] [--launches 12] [--skip-epilogue]

  train_pls  microseconds per iteration at the three `reference_scale` shapes of bench.py, (N, M, J) = (100, 10, 64),
             (1000, 32, 100), (4096, 128, 512), on both bases, for
               gamma/exp                  GammaCost / ExponentialLinkFunction: the library's fused routes
               negative_binomial/exp      the baseline: strictly more per element (a logarithm or a division on top of the
                                          exponential).  Measured TWICE per case, before and after the others: the ratio of
                                          the two runs is the baseline's own run-to-run spread, which the gamma ratio is read
                                          against
               poisson/square, bernoulli/sigmoid
               torch gamma                the same formulas as a torch PLSCost subclass, which train_pls runs through
                                          the un-fused entries (forward -> torch code -> particle update): what a user has
                                          without the library's cost
  epilogue   one large-rank step row: the forward GEMM with the cost-derivative epilogue on the plain route (PLS_OPT_WINOGRAD 0;
             timeline tag gemm_cost_deriv; the back-projection gemm_store beside it) at N = 50 000, M_k = 2048, J = 1024 for
             gamma/exp, negative_binomial/exp and bernoulli/sigmoid, alternating: the epilogue's price in ns per element of F
             and its share of the step's two contractions

One JSON line per case, then one summary line per block with the ratios.  train_pls: step + energy + early-stop test, the
median, minimum and maximum over --repeats runs of --iterations iterations, each run ended by a device synchronise; 30 warm-up
iterations per case.  epilogue: device time per launch from the library's event timeline, median / min / max over --launches
launches after three warm-up launches."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

SHAPES = ((100, 10, 64, 1), (1000, 32, 100, 1), (4096, 128, 512, 4))
EPILOGUE_SHAPES = ((50000, 2048, 1024),)
CONCENTRATION, DISPERSION = 4.0, 4.0


def stats(xs, digits=2):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def epilogue(args, torch, pkg):
    from projected_langevin_sampling_amd import _lib as L
    from projected_langevin_sampling_amd.basis import NoiseSpec, OrthonormalBasis
    from projected_langevin_sampling_amd.costs import BernoulliCost, GammaCost, NegativeBinomialCost
    from projected_langevin_sampling_amd.link_functions import ExponentialLinkFunction, SigmoidLinkFunction

    L.check(L.load().pls_set_option(L.OPT_WINOGRAD, 0), "pls_set_option")
    for n, mk, j in EPILOGUE_SHAPES:
        torch.manual_seed(0)
        a = torch.randn(mk, n, dtype=torch.float64, device="cuda") / mk ** 0.5
        lam = torch.rand(mk, dtype=torch.float64, device="cuda") + 0.5
        basis = OrthonormalBasis.from_projection(a, lam)
        basis.workspace_bytes = 8 << 30
        u = torch.randn(mk, j, dtype=torch.float64, device="cuda")
        out = torch.empty_like(u)
        y = torch._standard_gamma(torch.full((n,), CONCENTRATION)) / CONCENTRATION
        costs = {"gamma/exp": GammaCost(y, ExponentialLinkFunction(), concentration=CONCENTRATION),
                 "negative_binomial/exp": NegativeBinomialCost(torch.poisson(y + 0.5), ExponentialLinkFunction(), DISPERSION),
                 "bernoulli/sigmoid": BernoulliCost((y > 1).double(), SigmoidLinkFunction())}
        times = {name: {"gemm_cost_deriv": [], "gemm_store": []} for name in costs}

        def step(cost):
            basis.fused_step(cost, u, 1e-9, out=out, new_state=True, noise=NoiseSpec(none=True), force_generic=True)

        for cost in costs.values():
            for _ in range(3):
                step(cost)
        torch.cuda.synchronize()
        for _ in range(args.launches):  # alternating: the pairs see the same clocks
            for name, cost in costs.items():
                with L.Timeline(capacity=64) as tl:
                    step(cost)
                s = tl.summary()
                for tag in times[name]:
                    times[name][tag].append(s[tag]["avg_ms"] * s[tag]["launches"])
        med = {name: {tag: statistics.median(v) for tag, v in t.items()} for name, t in times.items()}
        whole = med["gamma/exp"]["gemm_cost_deriv"] + med["gamma/exp"]["gemm_store"]
        extra = {other: med["gamma/exp"]["gemm_cost_deriv"] - med[other]["gemm_cost_deriv"] for other in costs if other != "gamma/exp"}
        print(json.dumps({"label": args.label, "block": "epilogue", "n": n, "mk": mk, "j": j,
                          "forward_ms": {name: stats(t["gemm_cost_deriv"], 3) for name, t in times.items()},
                          "back_projection_ms": {name: stats(t["gemm_store"], 3) for name, t in times.items()},
                          "gamma_minus_other_ns_per_element": {o: round(v * 1e6 / (n * j), 4) for o, v in extra.items()},
                          "gamma_minus_other_share_of_step": {o: round(v / whole, 4) for o, v in extra.items()},
                          "forward_share_of_step": round(med["gamma/exp"]["gemm_cost_deriv"] / whole, 4), "launches": args.launches}), flush=True)
        del a, u, out, basis
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--skip-epilogue", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd import costs, link_functions
    from projected_langevin_sampling_amd.basis import InducingPointBasis, OrthonormalBasis
    from projected_langevin_sampling_amd.trainers import train_pls

    assert torch.cuda.is_available(), "gamma_cost_probe needs the GPU: there is no CPU timing"
    torch.set_default_dtype(torch.float64)

    class TorchGamma(costs.PLSCost):
        """what a user writes in torch where the library has no such cost"""

        def __init__(self, y_train, concentration):
            class Exp(link_functions.PLSLinkFunction):
                def transform(self, y):
                    return torch.exp(y)

            super().__init__(link_function=Exp(), observation_noise=None)
            self.y_train, self.k = y_train, float(concentration)
            self._z = torch.log(y_train).cuda()[:, None]

        def predict(self, prediction_samples):
            raise NotImplementedError

        def calculate_cost(self, untransformed_train_prediction_samples):
            t = self._z - untransformed_train_prediction_samples
            return self.k * (torch.exp(t) - t).sum(dim=0)

        def calculate_cost_derivative(self, untransformed_train_prediction_samples, force_autograd=False):
            return -self.k * torch.expm1(self._z - untransformed_train_prediction_samples)

    exp_link = link_functions.ExponentialLinkFunction
    ratios = {"gamma_over_nb": [], "nb_repeat_over_nb": [], "torch_over_gamma": [], "gamma_over_poisson": [], "gamma_over_bernoulli": []}
    for n, m, j, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(n, d, generator=g) * 2 - 1
        z = x[torch.randperm(n, generator=g)[:m]].clone()
        fstar = torch.sin(2.0 * x.sum(dim=1))
        y = torch.exp(fstar) * torch._standard_gamma(torch.full((n,), CONCENTRATION), generator=g) / CONCENTRATION
        y_count = torch.poisson(torch.exp(fstar) + 0.5, generator=g)
        kern = pkg.PLSKernel(pkg.ARDKernel(torch.full((d,), 0.5), 1.0), z)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bases = (("orthonormal", OrthonormalBasis(kern, z, x, 1e-8, verbose=False)), ("inducing_point", InducingPointBasis(kern, z, fstar[:m], x)))
        for bname, basis in bases:
            cases = [("negative_binomial/exp", costs.NegativeBinomialCost(y_count, exp_link(), DISPERSION)),
                     ("gamma/exp", costs.GammaCost(y, exp_link(), concentration=CONCENTRATION)),
                     ("poisson/square", costs.PoissonCost(y_count, link_functions.SquareLinkFunction())),
                     ("bernoulli/sigmoid", costs.BernoulliCost((fstar > 0).double(), link_functions.SigmoidLinkFunction())),
                     ("negative_binomial/exp (repeat)", costs.NegativeBinomialCost(y_count, exp_link(), DISPERSION)),
                     ("torch gamma", TorchGamma(y, CONCENTRATION))]
            u = (0.1 * torch.randn(basis.approximation_dimension, j, generator=g)).cuda()
            eta = 1e-13  # (timing only, as bench.py's block: inside every stability bound, so no run stops early)
            med = {}
            for name, cost in cases:
                assert cost.is_native() == (name != "torch gamma")
                pls = pkg.PLS(basis, cost)
                train_pls(pls, u.clone(), 30, eta, 1e9)
                runs = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, e = train_pls(pls, u.clone(), args.iterations, eta, 1e9)
                    torch.cuda.synchronize()
                    assert len(e) == args.iterations
                    runs.append((time.perf_counter() - t0) / args.iterations * 1e6)
                med[name] = statistics.median(runs)
                print(json.dumps({"label": args.label, "block": "train_pls", "cost": name, "n": n, "m": m, "j": j, "basis": bname,
                                  "us_per_iteration": stats(runs), "iterations": args.iterations, "repeats": args.repeats}), flush=True)
            row = {"gamma_over_nb": med["gamma/exp"] / med["negative_binomial/exp"],
                   "nb_repeat_over_nb": med["negative_binomial/exp (repeat)"] / med["negative_binomial/exp"],
                   "torch_over_gamma": med["torch gamma"] / med["gamma/exp"],
                   "gamma_over_poisson": med["gamma/exp"] / med["poisson/square"],
                   "gamma_over_bernoulli": med["gamma/exp"] / med["bernoulli/sigmoid"]}
            for key, v in row.items():
                ratios[key].append(v)
            print(json.dumps({"label": args.label, "block": "ratios", "n": n, "m": m, "j": j, "basis": bname,
                              **{key: round(v, 3) for key, v in row.items()}}), flush=True)
    print(json.dumps({"label": args.label, "block": "ratio ranges over the six cases",
                      **{key: [round(min(v), 3), round(max(v), 3)] for key, v in ratios.items()}}), flush=True)
    if not args.skip_epilogue:
        epilogue(args, torch, pkg)


if __name__ == "__main__":
    main()
