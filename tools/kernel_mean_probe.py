"""Time the exact-GP predictive mean two ways, in one process, through the package's library:

    python tools/kernel_mean_probe.py [--reps 30] [--warmup 3] [--models 5]

  fused         pls_kernel_mean: out = c + s sum_j kappa(x*_i, x_j) alpha_j, no matrix
  materialised  pls_kernel_gram into an n x t plane, then pls_gemm_tn (plane^T alpha): what ExactGP.predict does for its mean

for RBF, Matern-5/2, the rational-quadratic kernel (alpha = ln 2), the periodic kernel (lengthscales (0.5 + U) d, period
lengths 0.5 + 2.5 U), the locally periodic kernel (the periodic kernel's parameters under envelope lengthscales
(1 + U) sqrt(d)) and the trend-plus-seasonal kernel (the locally periodic kernel as the seasonal term, s_s = 0.9, under trend
lengthscales (2 + U) sqrt(d)) at (n, t, d) = (500, 1000, 1), (2000, 6500, 8), (5000, 36000, 8).  After a warm-up of each route the
timed calls alternate between the routes, each between its own pair of HIP events on torch's stream (the protocol of
tools/matern_gram_probe.py), so that drifts of clock or temperature fall on both alike.  Prints per route the median and
the 10th-90th percentile, the largest |fused - materialised| relative to the outputscale, the peak device memory of each
route (torch.cuda.max_memory_allocated above the inputs), whether the fused median lies below the materialised p10, the
wall time of one whole estimate_student_parameters with ``--models`` ExactGPs at the last shape, and a JSON line."""
import argparse
import json
import statistics
import time

import torch

import projected_langevin_sampling_amd as pkg

L = pkg._lib
KINDS = {L.KERNEL_RBF_ARD: "rbf", L.KERNEL_MATERN52: "matern52", L.KERNEL_RQ: "rq", L.KERNEL_PERIODIC: "periodic",
         L.KERNEL_LOCALLY_PERIODIC: "locally_periodic", L.KERNEL_TREND_SEASONAL: "trend_seasonal"}
SHAPES = [(500, 1000, 1), (2000, 6500, 8), (5000, 36000, 8)]
S, MEAN = 1.7, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", type=int, default=5)
    args = ap.parse_args()
    lib = L.load()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    result = {"reps": args.reps, "shapes": []}
    for n, t, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, d, generator=g, dtype=torch.float64).cuda()
        xt = torch.randn(t, d, generator=g, dtype=torch.float64).cuda()
        ls = (0.5 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5
        alpha = torch.randn(n, generator=g, dtype=torch.float64).cuda()
        lam = (0.5 + torch.rand(d, generator=g, dtype=torch.float64)) * d
        period = 0.5 + 2.5 * torch.rand(d, generator=g, dtype=torch.float64)
        envelope = (1.0 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5
        kernels = [pkg.ARDKernel(ls), pkg.MaternKernel(ls, nu=2.5), pkg.RQKernel(ls, alpha=0.6931471805599453),
                   pkg.PeriodicKernel(lam, period_length=period),
                   pkg.LocallyPeriodicKernel(envelope, periodic_lengthscale=lam, period_length=period)]
        trend = (2.0 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5  # (drawn last: the other kernels keep their draws)
        kernels.append(pkg.TrendSeasonalKernel(trend, seasonal_lengthscale=envelope, periodic_lengthscale=lam, period_length=period,
                                               seasonal_outputscale=0.9))
        for kernel in kernels:
            kind, kind_name = kernel.kind, KINDS[kernel.kind]
            ls = kernel._lengthscale_host(d).cuda()  # (the lengthscales, then the family's shape values)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            floor = torch.cuda.memory_allocated()
            fused_out = torch.empty(t, dtype=torch.float64, device="cuda")

            def fused():
                L.check(lib.pls_kernel_mean(kind, x.data_ptr(), n, d, ls.data_ptr(), S, MEAN, alpha.data_ptr(), xt.data_ptr(), t,
                                            fused_out.data_ptr(), sp), "pls_kernel_mean")

            fused()
            torch.cuda.synchronize()
            peak_fused = torch.cuda.max_memory_allocated() - floor
            torch.cuda.reset_peak_memory_stats()
            plane = torch.empty((n, t), dtype=torch.float64, device="cuda")
            mat_out = torch.empty((t, 1), dtype=torch.float64, device="cuda")

            def materialised():
                L.check(lib.pls_kernel_gram(kind, x.data_ptr(), n, xt.data_ptr(), t, d, ls.data_ptr(), S, plane.data_ptr(), t, sp),
                        "pls_kernel_gram")
                L.check(lib.pls_gemm_tn(plane.data_ptr(), t, alpha.data_ptr(), 1, mat_out.data_ptr(), 1, t, 1, n, 1.0, 0.0, sp),
                        "pls_gemm_tn")

            materialised()
            torch.cuda.synchronize()
            peak_mat = torch.cuda.max_memory_allocated() - floor
            diff = ((fused_out - (mat_out[:, 0] + MEAN)).abs().max() / S).item()
            routes = {"fused": fused, "materialised": materialised}
            for f in routes.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            ev = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, f in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f()
                    e1.record(stream)
                    ev[name].append((e0, e1))
            torch.cuda.synchronize()
            row = dict(n=n, t=t, d=d, kind=kind_name, max_diff_rel_s=diff, peak_bytes_fused=peak_fused, peak_bytes_materialised=peak_mat)
            for name in routes:
                ms = sorted(a.elapsed_time(b) for a, b in ev[name])
                row[name] = dict(median_ms=statistics.median(ms), p10_ms=ms[len(ms) // 10], p90_ms=ms[(9 * len(ms)) // 10],
                                 min_ms=ms[0], max_ms=ms[-1])
                print(f"n={n} t={t} d={d} {kind_name:>8} {name:>12}: median {row[name]['median_ms']:.4f} ms  p10-p90 "
                      f"{row[name]['p10_ms']:.4f}-{row[name]['p90_ms']:.4f}  min {ms[0]:.4f} max {ms[-1]:.4f}", flush=True)
            row["fused_median_below_materialised_p10"] = row["fused"]["median_ms"] < row["materialised"]["p10_ms"]
            print(f"n={n} t={t} d={d} {kind_name:>8}: fused / materialised median {row['fused']['median_ms'] / row['materialised']['median_ms']:.3f}; "
                  f"fused median < materialised p10: {row['fused_median_below_materialised_p10']}; |fused - materialised| / s {diff:.2e}; "
                  f"peak memory above the inputs: fused {peak_fused / 2**20:.2f} MiB, materialised {peak_mat / 2**20:.2f} MiB", flush=True)
            result["shapes"].append(row)
            del plane
    # one whole estimate_student_parameters: `models` ExactGPs on n-point subsamples predict at all t points
    n, t, d = SHAPES[-1]
    g = torch.Generator().manual_seed(1)
    xa = torch.randn(t, d, generator=g, dtype=torch.float64)
    ya = torch.sin(xa.sum(dim=1)) + 0.1 * torch.from_numpy(__import__("numpy").random.RandomState(0).standard_t(4.0, size=t))
    models = []
    for k in range(args.models):
        idx = torch.randperm(t, generator=g)[:n]
        models.append(pkg.ExactGP(xa[idx], ya[idx], "matern52"))
    xa_dev = xa.cuda()
    for phase in ("first call (factorisations)", "second call (alpha cached)"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        means = [m.predict_mean(xa_dev) for m in models]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nu, s = pkg.estimate_student_parameters(ya, means)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"estimate_student_parameters, {args.models} models, n={n} t={t} d={d}, {phase}: means {t1 - t0:.3f} s, "
              f"averaging and fit {t2 - t1:.3f} s -> nu {nu:.4f} scale {s:.4f}", flush=True)
        result.setdefault("estimate", []).append(dict(phase=phase, means_s=t1 - t0, fit_s=t2 - t1, nu=nu, scale=s))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
