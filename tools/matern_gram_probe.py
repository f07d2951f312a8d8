"""Time pls_kernel_gram per kernel kind through the C ABI, for one or more builds of libplship side by side.

    python tools/matern_gram_probe.py NAME=path/to/libplship.so [NAME=path ...] [--reps 40] [--warmup 3]

Shapes: k(Z, X) of configs[1] (1024 x 1e5, D = 8) and of configs[2] (512 x 5e4, D = 8).  Every library is loaded into this
one process (ctypes, RTLD_LOCAL); the RBF-ARD kind is timed for all of them, the Matern kinds for those whose ABI version is
7 or later, the rational-quadratic kind (alpha = ln 2, behind the lengthscales) for those that export the kind-aware workspace queries,
the periodic kind (period lengths 0.5 + 2.5 U behind the lengthscales) for those that do not call kind 8 unknown, the locally
periodic kind (the same periodic parameters behind envelope lengthscales (1 + U) sqrt(D)) for those that do not call kind 10
unknown, the trend-plus-seasonal kind (the locally periodic parameters behind trend lengthscales (2 + U) sqrt(D), s_s = 0.9) for
those that do not call kind 12 unknown.  After a warm-up of each (library, kind), the timed launches go round-robin over all (library, kind) pairs, each
between its own pair of HIP events on torch's stream, so that drifts of clock or temperature fall on every pair alike.
Prints one line per pair (median, 10th-90th percentile, min, max, median / first library's RBF median) and a JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from projected_langevin_sampling_amd import kernel as K  # noqa: E402  (parameter holders only: no library is loaded through it)

KINDS = {0: "rbf", 2: "matern12", 3: "matern32", 4: "matern52", 6: "rq", 8: "periodic", 10: "locally_periodic", 12: "trend_seasonal"}
SHAPES = [("configs[1] k(Z,X)", 1024, 100_000, 8), ("configs[2] k(Z,X)", 512, 50_000, 8)]


def load(path):
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    lib.pls_abi_version.restype = C.c_int
    lib.pls_last_error.restype = C.c_char_p
    lib.pls_kernel_gram.restype = C.c_int
    lib.pls_kernel_gram.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_double,
                                    C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NAME=path of a libplship build (the first is the baseline)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    libs = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        lib = load(path)
        kinds = [0] + ([2, 3, 4] if lib.pls_abi_version() >= 7 else []) + ([6] if hasattr(lib, "pls_gp_mll_workspace_bytes_kind") else [])
        for kind in (8, 10, 12):
            lib.pls_kernel_gram(kind, 8, 1, 8, 1, 1, None, 1.0, 8, 1, None)  # (refused before any launch: unknown, or "needs lengthscale")
            kinds += [kind] if b"unknown" not in lib.pls_last_error() else []
        libs.append((name, lib, kinds))
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    result = {"reps": args.reps, "shapes": []}
    for label, n1, n2, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        z = (torch.rand(n1, d, generator=g, dtype=torch.float64) * 2 - 1).cuda()
        x = (torch.rand(n2, d, generator=g, dtype=torch.float64) * 2 - 1).cuda()
        ls = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
        period = 0.5 + 2.5 * torch.rand(d, generator=g, dtype=torch.float64)
        envelope = (1.0 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5
        kernels = [K.ARDKernel(ls)] + [K.MaternKernel(ls, nu=nu) for nu in (0.5, 1.5, 2.5)] + [
            K.RQKernel(ls, alpha=0.6931471805599453), K.PeriodicKernel(ls, period_length=period),
            K.LocallyPeriodicKernel(envelope, periodic_lengthscale=ls, period_length=period)]
        trend = (2.0 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5  # (drawn last: the other kinds keep their draws)
        kernels.append(K.TrendSeasonalKernel(trend, seasonal_lengthscale=envelope, periodic_lengthscale=ls, period_length=period,
                                             seasonal_outputscale=0.9))
        params = {k.kind: k._lengthscale_host(d).cuda() for k in kernels}  # (per kind: the lengthscales, then its shape values)
        out = torch.empty(n1, n2, dtype=torch.float64, device="cuda")
        pairs = [(name, lib, kind) for name, lib, kinds in libs for kind in kinds]

        def launch(lib, kind):
            rc = lib.pls_kernel_gram(kind, z.data_ptr(), n1, x.data_ptr(), n2, d, params[kind].data_ptr(), 1.7,
                                     out.data_ptr(), n2, sp)
            if rc:
                raise RuntimeError(f"pls_kernel_gram(kind {kind}): {lib.pls_last_error().decode()}")

        for _, lib, kind in pairs:
            for _ in range(args.warmup):
                launch(lib, kind)
        torch.cuda.synchronize()
        ev = {(name, kind): [] for name, _, kind in pairs}
        for _ in range(args.reps):
            for name, lib, kind in pairs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(lib, kind)
                e1.record(stream)
                ev[(name, kind)].append((e0, e1))
        torch.cuda.synchronize()
        base = None
        rows = []
        for name, _, kind in pairs:
            ms = sorted(a.elapsed_time(b) for a, b in ev[(name, kind)])
            med = statistics.median(ms)
            if base is None:
                base = med
            p10, p90 = ms[len(ms) // 10], ms[(9 * len(ms)) // 10]
            row = dict(lib=name, kind=KINDS[kind], median_ms=med, p10_ms=p10, p90_ms=p90, min_ms=ms[0], max_ms=ms[-1],
                       vs_baseline_rbf=med / base, write_tb_s=8.0 * n1 * n2 / (med * 1e-3) / 1e12)
            rows.append(row)
            print(f"{label} {n1}x{n2} D={d}  {name:>8} {KINDS[kind]:>9}: median {med:.4f} ms  p10-p90 {p10:.4f}-{p90:.4f}  "
                  f"min {ms[0]:.4f} max {ms[-1]:.4f}  x{med / base:.3f} of {pairs[0][0]} rbf  ({row['write_tb_s']:.2f} TB/s written)",
                  flush=True)
        result["shapes"].append(dict(shape=label, n1=n1, n2=n2, d=d, rows=rows))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
