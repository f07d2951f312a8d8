"""Where an eigendecomposition of k(Z,Z) / M should run: host LAPACK, rocSOLVER (torch.linalg.eigh on the device) and
libplship's own solver (pls_sym_eigh, eigh_device="plship") on the same RBF Gram matrices, in one run.

Per size: the median and the fastest of REPS calls after a warm-up call per route, each closed by a device synchronise
(host clock), and each route's residual max|G V - V L| / ||G||_2 in units of eps.  With --setup the OrthonormalBasis
construction at the benchmark's M = 1024 follows on all three routes.  profiles/sym_eigh.txt is a run of
    python tools/eigh_probe.py --setup
The earlier large-size table (M = 1024, 2048, 4096; host against rocSOLVER only) is `--sizes 1024 2048 4096 --no-plship`."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = 2.0 ** -52


def gram(m):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 2, dtype=torch.float64, generator=g)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return torch.exp(-d / (2 * 0.6 ** 2)) / m


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out) * 1e3, min(out) * 1e3, r


def residual(g, lam, vec):
    g, lam, vec = g.cpu(), lam.cpu(), vec.cpu()
    return float(((g @ vec) - vec * lam[None, :]).abs().max() / lam.abs().max() / EPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 32, 64, 100, 128, 256, 512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-plship", action="store_true")
    ap.add_argument("--setup", action="store_true", help="also time OrthonormalBasis at M = 1024, N = 36000 on every route")
    args = ap.parse_args()
    from projected_langevin_sampling_amd import _ops
    from projected_langevin_sampling_amd.samplers import host_eigh

    assert torch.cuda.is_available(), "the probe measures the device routes: it needs the GPU"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {torch.get_num_threads()} host threads; {args.reps} calls per "
          "figure after one warm-up call; ms = median (fastest); residual in eps ||G||_2")
    print(f"{'M':>6} | {'host LAPACK':>22} {'res':>6} | {'rocSOLVER':>22} {'res':>6} | {'plship':>22} {'res':>6} {'info':>4}")
    for m in args.sizes:
        g = gram(m)
        gd = g.cuda()
        reps = args.reps if m <= 1024 else 2
        th = timed(lambda: host_eigh(g), reps)
        tr = timed(lambda: torch.linalg.eigh(gd), reps)
        row = (f"{m:>6} | {th[0]:>10.3f} ({th[1]:>9.3f}) {residual(g, *th[2]):>6.1f} | {tr[0]:>10.3f} ({tr[1]:>9.3f}) "
               f"{residual(g, *tr[2]):>6.1f} | ")
        if not args.no_plship:
            tp = timed(lambda: _ops.sym_eigh(gd, return_info=True), reps)
            row += f"{tp[0]:>10.3f} ({tp[1]:>9.3f}) {residual(g, tp[2][0], tp[2][1]):>6.1f} {tp[2][2]:>4}"
        print(row, flush=True)
    if args.setup:
        import projected_langevin_sampling_amd as pkg
        from projected_langevin_sampling_amd.basis import OrthonormalBasis

        gen = torch.Generator().manual_seed(0)
        n, m, d = 36000, 1024, 8
        x = torch.rand(n, d, dtype=torch.float64, generator=gen) * 2 - 1
        z = x[:m].clone()
        ls = torch.full((d,), 1.5, dtype=torch.float64)
        print(f"# OrthonormalBasis setup, N = {n}, M = {m}, d = {d} (threshold 1e-10): seconds per phase, second of two constructions")
        for route in ("cpu", "cuda", "plship"):
            for rep in range(2):
                times = {}
                t0 = time.perf_counter()
                b = OrthonormalBasis(pkg.PLSKernel(pkg.ARDKernel(ls, 1.0), z), z, x, 1e-10, verbose=False, eigh_device=route,
                                     setup_times=times)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
            phases = "  ".join(f"{k} {v:.4f}" for k, v in times.items())
            print(f"{route:>7}: total {total:.4f} s  ({phases})  kept {b.approximation_dimension}", flush=True)


if __name__ == "__main__":
    main()
