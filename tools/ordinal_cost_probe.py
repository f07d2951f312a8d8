#!/usr/bin/env python3
"""Times the ordinal cost (cumulative logit, identity link).

    python tools/ordinal_cost_probe.py --variant native|unfused|bernoulli [--root TREE] [--iterations 200] [--repeats 7]
    python tools/ordinal_cost_probe.py --variant epilogue [--launches 12]

  native     OrdinalCost / IdentityLinkFunction (four categories, cutpoints from the labels) through train_pls at the three
             `reference_scale` shapes of bench.py, (N, M, J) = (100, 10, 64), (1000, 32, 100), (4096, 128, 512), on both bases
             (the shapes of profiles/negative_binomial_cost.txt): the library's fused routes
  unfused    the only way a build without the cost offers it: a torch PLSCost subclass with the same formulas, which
             train_pls runs through pls_onb_forward / pls_ipb_forward -> torch code -> the particle update.  Needs nothing of
             the new cost, so --root may point at a checkout (and build) of the commit before it
  bernoulli  Bernoulli/sigmoid on the same problem (labels cut at the middle): one softplus term where the ordinal cost has two
  epilogue   the forward GEMM with the cost-derivative epilogue on the plain route (PLS_OPT_WINOGRAD 0; timeline tag
             gemm_cost_deriv; the back-projection is timed beside it), ordinal/identity against Bernoulli/sigmoid in one
             process, alternating, at a shard-sized large-rank shape (N = 50 000, M_k = 2048, J = 1024): the difference is the
             price of the second term, stated in ns per element of F and as a share of the step's two contractions

One JSON line per case.  train_pls: microseconds per iteration (step + energy + early-stop test), the median, minimum and
maximum over --repeats runs of --iterations iterations, each run ended by a device synchronise; 30 warm-up iterations per
case.  epilogue: device time per launch from the library's event timeline, median / min / max over --launches launches after
three warm-up launches.  Compare variants from processes started in turn in one session (the host is shared: see the spread)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

SHAPES = ((100, 10, 64, 1), (1000, 32, 100, 1), (4096, 128, 512, 4))
EPILOGUE_SHAPES = ((50000, 2048, 1024),)
THRESHOLDS = (-0.75, 0.0, 0.75)  # four grades cut from the noisy latent


def stats(xs, digits=2):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def epilogue(args, torch, pkg):
    from projected_langevin_sampling_amd import _lib as L
    from projected_langevin_sampling_amd.basis import NoiseSpec, OrthonormalBasis
    from projected_langevin_sampling_amd.costs import BernoulliCost, OrdinalCost
    from projected_langevin_sampling_amd.link_functions import IdentityLinkFunction, SigmoidLinkFunction

    L.check(L.load().pls_set_option(L.OPT_WINOGRAD, 0), "pls_set_option")

    for n, mk, j in EPILOGUE_SHAPES:
        torch.manual_seed(0)
        a = torch.randn(mk, n, dtype=torch.float64, device="cuda") / mk ** 0.5
        lam = torch.rand(mk, dtype=torch.float64, device="cuda") + 0.5
        basis = OrthonormalBasis.from_projection(a, lam)
        basis.workspace_bytes = 8 << 30
        u = torch.randn(mk, j, dtype=torch.float64, device="cuda")
        out = torch.empty_like(u)
        labels = torch.randint(0, 4, (n,)).double()
        costs = {"ordinal/identity": OrdinalCost(labels, IdentityLinkFunction(), OrdinalCost.cutpoints_from_labels(labels)),
                 "bernoulli/sigmoid": BernoulliCost((labels >= 2).double(), SigmoidLinkFunction())}
        times = {name: {"gemm_cost_deriv": [], "gemm_store": []} for name in costs}

        def step(cost):
            basis.fused_step(cost, u, 1e-9, out=out, new_state=True, noise=NoiseSpec(none=True), force_generic=True)

        for cost in costs.values():
            for _ in range(3):
                step(cost)
        torch.cuda.synchronize()
        for _ in range(args.launches):  # alternating: both pairs see the same clocks
            for name, cost in costs.items():
                with L.Timeline(capacity=64) as tl:
                    step(cost)
                s = tl.summary()
                for tag in times[name]:
                    times[name][tag].append(s[tag]["avg_ms"] * s[tag]["launches"])
        med = {name: {tag: statistics.median(v) for tag, v in t.items()} for name, t in times.items()}
        extra_ms = med["ordinal/identity"]["gemm_cost_deriv"] - med["bernoulli/sigmoid"]["gemm_cost_deriv"]
        whole = med["ordinal/identity"]["gemm_cost_deriv"] + med["ordinal/identity"]["gemm_store"]
        print(json.dumps({"label": args.label, "variant": "epilogue", "n": n, "mk": mk, "j": j,
                          "forward_ms": {name: stats(t["gemm_cost_deriv"], 3) for name, t in times.items()},
                          "back_projection_ms": {name: stats(t["gemm_store"], 3) for name, t in times.items()},
                          "ordinal_minus_bernoulli_ns_per_element": round(extra_ms * 1e6 / (n * j), 4),
                          "ordinal_minus_bernoulli_share_of_step": round(extra_ms / whole, 4), "launches": args.launches}), flush=True)
        del a, u, out, basis
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("native", "unfused", "bernoulli", "epilogue"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd import costs, link_functions
    from projected_langevin_sampling_amd.basis import InducingPointBasis, OrthonormalBasis
    from projected_langevin_sampling_amd.trainers import train_pls

    assert torch.cuda.is_available(), "ordinal_cost_probe needs the GPU: there is no CPU timing"
    print(f"ordinal_cost_probe: package from {os.path.dirname(pkg.__file__)}", file=sys.stderr)
    torch.set_default_dtype(torch.float64)
    if args.variant == "epilogue":
        return epilogue(args, torch, pkg)

    class TorchOrdinal(costs.PLSCost):
        """what a user writes in torch where the library has no such cost"""

        def __init__(self, y_train, cutpoints):
            class Identity(link_functions.PLSLinkFunction):
                def transform(self, y):
                    return y

            super().__init__(link_function=Identity(), observation_noise=None)
            self.y_train = y_train
            b = torch.tensor([-float("inf")] + list(cutpoints) + [float("inf")])
            k = y_train.long()
            self._lo, self._hi = b[k].cuda()[:, None], b[k + 1].cuda()[:, None]

        def predict(self, prediction_samples):
            raise NotImplementedError

        def calculate_cost(self, untransformed_train_prediction_samples):
            f = untransformed_train_prediction_samples
            zero = torch.zeros_like(f)
            return (torch.logaddexp(zero, f - self._hi) + torch.logaddexp(zero, self._lo - f)).sum(dim=0)

        def calculate_cost_derivative(self, untransformed_train_prediction_samples, force_autograd=False):
            f = untransformed_train_prediction_samples
            return torch.sigmoid(f - self._hi) - torch.sigmoid(self._lo - f)

    for n, m, j, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(n, d, generator=g) * 2 - 1
        z = x[torch.randperm(n, generator=g)[:m]].clone()
        fstar = torch.sin(2.0 * x.sum(dim=1))
        uniform = torch.rand(n, generator=g).clamp(1e-12, 1 - 1e-12)
        latent = 1.5 * fstar + torch.log(uniform) - torch.log1p(-uniform)  # logistic noise
        y = torch.bucketize(latent, torch.tensor(THRESHOLDS)).double()
        counts = torch.bincount(y.long(), minlength=4).double() + 0.5  # (cutpoints_from_labels, restated: --root may predate it)
        cum = torch.cumsum(counts, 0)[:-1] / counts.sum()
        cutpoints = (torch.log(cum) - torch.log1p(-cum)).tolist()
        kern = pkg.PLSKernel(pkg.ARDKernel(torch.full((d,), 0.5), 1.0), z)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bases = (("orthonormal", OrthonormalBasis(kern, z, x, 1e-8, verbose=False)), ("inducing_point", InducingPointBasis(kern, z, fstar[:m], x)))
        for bname, basis in bases:
            if args.variant == "native":
                cost = costs.OrdinalCost(y, link_functions.IdentityLinkFunction(), cutpoints=cutpoints)
                assert cost.is_native()
            elif args.variant == "unfused":
                cost = TorchOrdinal(y, cutpoints)
                assert not cost.is_native()
            else:
                cost = costs.BernoulliCost((y >= 2).double(), link_functions.SigmoidLinkFunction())
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
                              "us_per_iteration": stats(runs), "iterations": args.iterations, "repeats": args.repeats}), flush=True)


if __name__ == "__main__":
    main()
