"""Do two builds of libplship give the same bits from the pairwise base-kernel entries?

    python tools/base_kernel_same.py A=path/to/libplship.so B=path/to/libplship.so

Both libraries are loaded into this one process (ctypes, RTLD_LOCAL, as tools/matern_gram_probe.py) and called on identical
device inputs; the outputs are compared with torch.equal.  pls_kernel_gram: the five kinds of ABI 7 (RBF, linear,
Matern; an entry that one of the builds lacks is not called), every D_MAX padded and exact,
(65, 515) and (1, 1), both store paths; pls_kernel_grad_sums: the stationary kinds, n = 130 and 515, both ldp parities;
pls_kernel_mean: the sizes and dimensions of tests/test_gpu_kernel_mean.py, aligned and 8-byte-offset inputs;
pls_gp_mll_grad: the three cases of test_model_evaluation_is_gp_mll_grad, without and with jitter.  The inputs hold one
duplicated point and one point 1e4 lengthscales away.  Prints one row per entry -- calls, differing elements -- and exits
non-zero on any difference."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_gp_truth as T  # noqa: E402
import projected_langevin_sampling_amd as pkg  # noqa: E402

F64 = torch.float64
DIMS = [1, 2, 3, 5, 8, 13, 33, 64]
NAN = float("nan")


def load(path):
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    for name, (res, args) in pkg._lib.SIGNATURES.items():
        if not hasattr(lib, name):  # (a build from before the entry existed: the comparison does not call it)
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def offset(m):
    """a device copy of m 8 bytes past a 16-byte boundary"""
    raw = torch.full((1 + m.numel(),), NAN, dtype=F64, device="cuda")
    raw[1:].view(m.shape).copy_(m)
    return raw[1:].view(m.shape)


def problem(n, m, d, seed):
    """x (n, d), xt (m, d) ~ N(0, 1), lengthscales (0.5 - 1.5) sqrt(d); xt[0] = x[0] and x[n - 1] 1e4 lengthscales away"""
    g = torch.Generator().manual_seed(seed)
    x, xt = torch.randn(n, d, generator=g, dtype=F64), torch.randn(m, d, generator=g, dtype=F64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
    xt[0] = x[0]
    x[n - 1] = x[n - 1] + 1e4 * ls
    if n > 2:
        x[1] = x[0]
    return x.cuda(), xt.cuda(), ls.cuda(), g


def check(lib, rc, what):
    if rc:
        raise RuntimeError(f"{what}: {lib.pls_last_error().decode()}")


def gram_calls(sp):
    for kind in (0, 1, 2, 3, 4):
        for d in DIMS:
            for n1, n2 in ((65, 515), (1, 1)):
                x1, x2, ls, _ = problem(n1, n2, d, 100 * d + kind + n1)
                for ldout, shift in ((n2 + n2 % 2, 0), (n2 + 1 - n2 % 2, 1)):  # even on 16 bytes; odd, 8 bytes off
                    def call(lib):
                        raw = torch.full((shift + n1 * ldout,), NAN, dtype=F64, device="cuda")
                        check(lib, lib.pls_kernel_gram(kind, x1.data_ptr(), n1, x2.data_ptr(), n2, d, ls.data_ptr(), 1.7,
                                                       raw[shift:].data_ptr(), ldout, sp), "pls_kernel_gram")
                        return raw
                    yield call


def grad_sums_calls(sp):
    for kind in T.KINDS:
        for d in DIMS:
            for n in (130, 515):
                x, _, ls, g = problem(n, 1, d, 200 * d + kind + n)
                alpha = torch.randn(n, generator=g, dtype=F64).cuda()
                a = torch.randn(n, n, generator=g, dtype=F64)
                for ldp, shift in ((n + n % 2, 0), (n + 1 - n % 2, 1)):
                    raw = torch.full((shift + n * ldp,), NAN, dtype=F64, device="cuda")
                    raw[shift:].view(n, ldp)[:, :n] = (a + a.T).cuda()

                    def call(lib, raw=raw, ldp=ldp, shift=shift):
                        nbytes = lib.pls_kernel_grad_sums_workspace_bytes(n, d)
                        ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
                        out = torch.full((d + 2,), NAN, dtype=F64, device="cuda")
                        check(lib, lib.pls_kernel_grad_sums(kind, x.data_ptr(), n, d, ls.data_ptr(), 1.7, alpha.data_ptr(),
                                                            raw[shift:].data_ptr(), ldp, out.data_ptr(), ws.data_ptr(), nbytes, sp),
                              "pls_kernel_grad_sums")
                        return out
                    yield call


def mean_calls(sp):
    sizes = [(n, t, 5) for n in (1, 2, 65, 515) for t in (1, 2, 65, 130)] + [(130, 70, d) for d in DIMS]
    for kind in T.KINDS:
        for n, t, d in sizes:
            x, xt, ls, g = problem(n, t, d, 300 * d + kind + 7 * n + t)
            alpha = torch.randn(n, generator=g, dtype=F64).cuda()
            for xd, xtd in ((x, xt), (offset(x), offset(xt))):
                def call(lib, xd=xd, xtd=xtd):
                    out = torch.full((t + 1,), NAN, dtype=F64, device="cuda")
                    check(lib, lib.pls_kernel_mean(kind, xd.data_ptr(), n, d, ls.data_ptr(), 1.7, 0.3, alpha.data_ptr(),
                                                   xtd.data_ptr(), t, out.data_ptr(), sp), "pls_kernel_mean")
                    return out
                yield call


def gp_mll_calls(sp):
    for name in ("rbf-n130-d3", "matern32-n65-d8", "matern52-n2-d1"):
        kind, x, y, ls = T.case_inputs(name)
        (n, d), x, y, ls = x.shape, x.cuda(), y.cuda(), ls.cuda()
        for jitter in (0.0, 1e-6):
            def call(lib, jitter=jitter):
                nbytes = lib.pls_gp_mll_workspace_bytes(n, d)
                ws = torch.full((nbytes // 8,), NAN, dtype=F64, device="cuda")
                out = torch.full((4 + d + 1,), NAN, dtype=F64, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                check(lib, lib.pls_gp_mll_grad(kind, x.data_ptr(), n, d, ls.data_ptr(), T.OUTPUTSCALE, T.NOISE, T.MEAN, jitter,
                                               y.data_ptr(), out.data_ptr(), info.data_ptr(), ws.data_ptr(), nbytes, sp),
                      "pls_gp_mll_grad")
                return out
            yield call


def main(specs):
    (name_a, a), (name_b, b) = [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in specs]
    torch.cuda.init()
    sp = torch.cuda.current_stream().cuda_stream
    bad = 0
    print(f"{name_a} against {name_b}\n{'entry':<24}{'calls':>8}{'elements':>12}{'differing':>11}")
    for entry, calls in (("pls_kernel_gram", gram_calls), ("pls_kernel_grad_sums", grad_sums_calls),
                         ("pls_kernel_mean", mean_calls), ("pls_gp_mll_grad", gp_mll_calls)):
        count = elements = differing = 0
        for call in calls(sp):
            ra, rb = call(a).cpu().view(torch.int64), call(b).cpu().view(torch.int64)  # bits: the NaN padding included
            count, elements, differing = count + 1, elements + ra.numel(), differing + int((ra != rb).sum())
        print(f"{entry:<24}{count:>8}{elements:>12}{differing:>11}")
        bad += differing
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1:]))
