"""Where one exact-GP marginal-likelihood evaluation (pls_gp_mll_grad) spends its time, and what the same value and
gradient cost through torch.linalg.cholesky + autograd in fp64 on the same card (the reference's route without
gpytorch's overhead).

    python tools/gp_mll_probe.py [--out profiles/gp_mll.txt] [--sizes 2000 5000] [--dims 2 8] [--repeats 5]

Per shape: the whole call, and the stages that are library entry points of their own -- Gram build (pls_kernel_gram),
factorisation (pls_chol_factor), solve (pls_chol_solve), inverse factor (pls_chol_build_inverse), reduction
(pls_kernel_grad_sums) -- each timed with device events around the call on warmed-up shapes, median of the repeats.  The
K_y^-1 = Linv^T Linv product runs inside the library as a triangular contraction with no entry point of its own: it is
reported as the remainder (whole call minus the stages above), which also holds the three small kernels (diagonal,
centring, finish).  Needs the MI355X; there is no fallback."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import projected_langevin_sampling_amd as pkg  # noqa: E402

L = pkg._lib
F64 = torch.float64
KINDS = {"rbf": L.KERNEL_RBF_ARD, "matern52": L.KERNEL_MATERN52, "rq": L.KERNEL_RQ, "periodic": L.KERNEL_PERIODIC,
         "locally_periodic": L.KERNEL_LOCALLY_PERIODIC, "trend_seasonal": L.KERNEL_TREND_SEASONAL}
RQ_ALPHA = math.log(2.0)  # behind the lengthscales in the library's array; its derivative is the last output


def timed(fn, repeats):
    """median milliseconds of fn() between two events (one warm-up call first)"""
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
    return statistics.median(ms)


def probe_kernel(kind, d, g):
    """The kernel whose parameters are timed: lengthscales (0.5 + U) sqrt(d), drawn for every kind; RQ: alpha = ln 2; periodic:
    lengthscales (0.5 + U) d and period lengths 0.5 + 2.5 U, drawn after them; locally periodic: the periodic kind's draws under
    envelope lengthscales (1 + U) sqrt(d), drawn last; trend plus seasonal: the locally periodic kind's draws as the seasonal
    term (s_s = 0.9) under trend lengthscales (2 + U) sqrt(d), drawn after them."""
    ls = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
    if kind in (L.KERNEL_PERIODIC, L.KERNEL_LOCALLY_PERIODIC, L.KERNEL_TREND_SEASONAL):
        lam, period = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d, 0.5 + 2.5 * torch.rand(d, generator=g, dtype=F64)
        if kind == L.KERNEL_PERIODIC:
            return pkg.PeriodicKernel(lam, period_length=period)
        envelope = (1.0 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
        if kind == L.KERNEL_TREND_SEASONAL:
            return pkg.TrendSeasonalKernel((2.0 + torch.rand(d, generator=g, dtype=F64)) * d**0.5, seasonal_lengthscale=envelope,
                                           periodic_lengthscale=lam, period_length=period, seasonal_outputscale=0.9)
        return pkg.LocallyPeriodicKernel(envelope, periodic_lengthscale=lam, period_length=period)
    return {L.KERNEL_RBF_ARD: pkg.ARDKernel(ls), L.KERNEL_MATERN52: pkg.MaternKernel(ls, nu=2.5), L.KERNEL_RQ: pkg.RQKernel(ls, alpha=RQ_ALPHA)}[kind]


def library_stages(kind, x, y, ls, s, noise, mean, repeats):
    lib = L.load()
    n, d = x.shape
    ld = (n + 1) // 2 * 2
    st = L.stream_ptr
    planes = [torch.empty((n, ld), dtype=F64, device="cuda") for _ in range(7)]
    ky, lc, lct, sf, sb, linv, linvt = planes
    r, alpha = (y - mean).contiguous(), torch.empty(n, dtype=F64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    extra = L.kernel_shape_params(kind, d)  # (shape values behind the lengthscales)
    assert ls.numel() == d + extra
    out = torch.empty(4 + d + extra, dtype=F64, device="cuda")
    nbytes = lib.pls_gp_mll_workspace_bytes_kind(kind, n, d)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    rbytes = lib.pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d)
    rws, sums = torch.empty(rbytes // 8 + 1, dtype=F64, device="cuda"), torch.empty(d + 1 + extra, dtype=F64, device="cuda")
    desc = L.CholDesc()
    desc.m = n
    desc.Lc, desc.ldlc, desc.LcT, desc.ldlct = lc.data_ptr(), ld, lct.data_ptr(), ld
    desc.Sf, desc.ldsf, desc.Sb, desc.ldsb = sf.data_ptr(), ld, sb.data_ptr(), ld

    def whole():
        L.check(lib.pls_gp_mll_grad(kind, x.data_ptr(), n, d, ls.data_ptr(), s, noise, mean, 0.0, y.data_ptr(), out.data_ptr(),
                                    info.data_ptr(), ws.data_ptr(), nbytes, st()), "pls_gp_mll_grad")

    def gram():
        L.check(lib.pls_kernel_gram(kind, x.data_ptr(), n, x.data_ptr(), n, d, ls.data_ptr(), s, ky.data_ptr(), ld, st()), "gram")

    def factor():
        L.check(lib.pls_chol_factor(ky.data_ptr(), ld, n, 0.0, lc.data_ptr(), ld, lct.data_ptr(), ld, sf.data_ptr(), ld,
                                    sb.data_ptr(), ld, info.data_ptr(), st()), "factor")

    def solve():
        L.check(lib.pls_chol_solve(desc, r.data_ptr(), 1, 1, alpha.data_ptr(), 1, st()), "solve")

    def inverse():
        L.check(lib.pls_chol_build_inverse(desc, linv.data_ptr(), ld, linvt.data_ptr(), ld, st()), "inverse")

    def reduction():  # (any symmetric P costs the same: the Gram plane stands in for K_y^-1)
        L.check(lib.pls_kernel_grad_sums(kind, x.data_ptr(), n, d, ls.data_ptr(), s, alpha.data_ptr(), ky.data_ptr(), ld,
                                         sums.data_ptr(), rws.data_ptr(), rbytes, st()), "reduction")

    res = {"whole": timed(whole, repeats)}
    assert int(info.item()) == 0, "the probe's matrix is not positive definite"
    res["gram"] = timed(gram, repeats)
    ky.diagonal().add_(noise)
    for name, fn in (("factor", factor), ("solve", solve), ("inverse", inverse)):
        res[name] = timed(fn, repeats)
    gram()
    res["reduction"] = timed(reduction, repeats)
    res["product+small"] = res["whole"] - sum(v for k, v in res.items() if k != "whole")
    return res, out.cpu()


def torch_route(kind, x, y, ls, s, noise, mean, repeats):
    """-> (ms, the same 4 + d + shape parameters numbers): value and gradient by autograd through torch.linalg.cholesky, fp64,
    same device"""
    n, d = x.shape
    leaves = [torch.tensor(v, dtype=F64, device="cuda", requires_grad=True) for v in (mean, noise, math.log(s))]
    log_ls = ls[:d].log().clone().requires_grad_(True)
    log_alpha = torch.tensor(math.log(RQ_ALPHA), dtype=F64, device="cuda", requires_grad=True)
    trend = kind == L.KERNEL_TREND_SEASONAL  # (l, m, lambda, p in blocks of d, then s_s; log_ls is then the trend's)
    local = kind == L.KERNEL_LOCALLY_PERIODIC or trend  # (l, lambda, p in blocks of d; log_ls is then the envelope's)
    o = d if trend else 0  # (where the locally periodic blocks start)
    log_p = (ls[o + 2 * d:o + 3 * d] if local else ls[d:2 * d] if kind == L.KERNEL_PERIODIC else ls[:d]).log().clone().requires_grad_(True)  # (periodic kinds only)
    log_lam = (ls[o + d:o + 2 * d] if local else ls[:d]).log().clone().requires_grad_(True)  # (locally periodic, trend plus seasonal)
    log_env = ls[o:o + d].log().clone().requires_grad_(True)  # (trend plus seasonal: the seasonal term's envelope)
    log_ss = ls[-1].log().clone().requires_grad_(True)  # (trend plus seasonal: the seasonal outputscale)
    result = {}

    def run():
        for t in leaves + [log_ls, log_alpha, log_p, log_lam, log_env, log_ss]:
            t.grad = None
        e2t = torch.zeros((n, n), dtype=F64, device="cuda")  # (trend plus seasonal: the trend's squared distance)
        e2 = torch.zeros((n, n), dtype=F64, device="cuda")
        for k in range(d):
            if kind == L.KERNEL_PERIODIC:  # (e2 holds the negated exponent, sum_k 2 sin^2(pi e_k) / lambda_k)
                e = (x[:, k][:, None] - x[:, k][None, :]) / log_p[k].exp()
                e2 = e2 + 2.0 * torch.sin(math.pi * e).square() / log_ls[k].exp()
                continue
            if local:  # (the negated exponent again, the envelope's share added)
                delta = x[:, k][:, None] - x[:, k][None, :]
                if trend:
                    e2t = e2t + (delta / log_ls[k].exp()).square()
                e2 = e2 + 0.5 * (delta / (log_env if trend else log_ls)[k].exp()).square() + 2.0 * torch.sin(math.pi * delta / log_p[k].exp()).square() / log_lam[k].exp()
                continue
            a = x[:, k] / log_ls[k].exp()
            e2 = e2 + (a[:, None] - a[None, :]).square()
        if kind == L.KERNEL_PERIODIC or local:
            kap = torch.exp(-e2)
        elif kind == L.KERNEL_RBF_ARD:
            kap = torch.exp(-0.5 * e2)
        elif kind == L.KERNEL_RQ:
            kap = torch.exp(-log_alpha.exp() * torch.log1p(e2 / (2.0 * log_alpha.exp())))
        else:  # sqrt has no derivative at 0: the diagonal is taken out before it
            off = ~torch.eye(n, dtype=torch.bool, device="cuda")
            t = torch.sqrt(5.0 * torch.where(off, e2, torch.ones_like(e2)))
            kap = torch.where(off, (1.0 + t + t * t / 3.0) * torch.exp(-t), torch.ones_like(e2))
        ky = leaves[2].exp() * (torch.exp(-0.5 * e2t) if trend else kap) + leaves[1] * torch.eye(n, dtype=F64, device="cuda")
        if trend:
            ky = ky + log_ss.exp() * kap
        low = torch.linalg.cholesky(ky)
        r = y - leaves[0]
        alpha = torch.cholesky_solve(r[:, None], low)[:, 0]
        mll = -0.5 * r @ alpha - torch.log(low.diagonal()).sum() - 0.5 * n * math.log(2.0 * math.pi)
        mll.backward()
        tail = [log_alpha.grad.reshape(1)] if kind == L.KERNEL_RQ else [log_p.grad] if kind == L.KERNEL_PERIODIC else [log_env.grad, log_lam.grad, log_p.grad, log_ss.grad.reshape(1)] if trend else [log_lam.grad, log_p.grad] if local else []
        result["out"] = torch.cat([mll.detach().reshape(1), torch.stack([t.grad for t in leaves]), log_ls.grad] + tail)

    return timed(run, repeats), result["out"].cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_mll.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 5000])
    ap.add_argument("--dims", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    lines = [f"# tools/gp_mll_probe.py on {torch.cuda.get_device_name(0)}: one exact-GP marginal-likelihood evaluation, milliseconds",
             f"# (device events, median of {args.repeats} after a warm-up call); product+small = whole - the other stages",
             "# torch = the same value and gradient by torch.linalg.cholesky + autograd, fp64, same card; agree = the largest",
             "# difference of the 4 + d outputs relative to the largest output",
             f"{'kind':16s} {'n':>5s} {'d':>2s} {'whole':>8s} {'gram':>7s} {'factor':>7s} {'solve':>7s} {'inverse':>7s} {'product+small':>13s} "
             f"{'reduction':>9s} {'red/whole':>9s} {'torch':>8s} {'torch/whole':>11s} {'agree':>8s}"]
    for name, kind in ((k, KINDS[k]) for k in args.kinds):
        for n in args.sizes:
            for d in args.dims:
                g = torch.Generator().manual_seed(n + d)
                x = torch.randn(n, d, generator=g, dtype=F64).cuda()
                y = (torch.sin(x.sum(dim=1)) + 0.3 * torch.randn(n, generator=g, dtype=F64).cuda()).contiguous()
                ls = probe_kernel(kind, d, g)._lengthscale_host(d).cuda()
                res, out = library_stages(kind, x, y, ls, 1.3, 0.1, 0.2, args.repeats)
                row = (f"{name:16s} {n:5d} {d:2d} {res['whole']:8.3f} {res['gram']:7.3f} {res['factor']:7.3f} {res['solve']:7.3f} "
                       f"{res['inverse']:7.3f} {res['product+small']:13.3f} {res['reduction']:9.3f} "
                       f"{res['reduction'] / res['whole']:9.3f}")
                try:
                    torch.cuda.empty_cache()
                    t_ms, t_out = torch_route(kind, x, y, ls, 1.3, 0.1, 0.2, args.repeats)
                    agree = ((out - t_out).abs().max() / t_out.abs().max()).item()
                    row += f" {t_ms:8.3f} {t_ms / res['whole']:11.2f} {agree:8.1e}"
                except RuntimeError as e:  # (the vendor BLAS behind autograd's triangular solves can refuse a size: say so)
                    row += f"  torch route not measured: {str(e).splitlines()[0][:90]}"
                lines.append(row)
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:5]))


if __name__ == "__main__":
    main()
