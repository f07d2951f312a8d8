"""What the per-family GPU files (test_gpu_rq.py, test_gpu_periodic.py, test_gpu_matern.py) share byte for byte: the calls of the
pairwise base-kernel entries through the C ABI and the buffers they are given.  Every wrapper takes the kernel kind and the
library's parameter vector (the d lengthscales, then _lib.kernel_shape_params(kind, d) shape values), puts a NaN canary
behind the last output and behind the workspace, and asserts that the canary survived.  The bars, the draws and the closed
forms stay in the family's own file.  ``P`` is the namespace fixture of test_gpu_parity."""
import torch

F64 = torch.float64


def cu(t):
    return t.to(device="cuda", dtype=F64)


def make_note():
    """-> note(test, tag, ratio): prints a case's err / bar and the largest of its test so far, per file that makes one"""
    worst = {}

    def note(test, tag, ratio):
        worst[test] = max(worst.get(test, 0.0), float(ratio))
        print(f"{test} {tag}: err/bar {float(ratio):.2e} (largest so far {worst[test]:.2e})")

    return note


def lib_params(ls, shape):
    """the doubles the library reads on the device: the lengthscales, then the shape values (a float or a tensor)"""
    return torch.cat([ls.double().reshape(-1), torch.as_tensor(shape, dtype=F64).reshape(-1)]).cuda().contiguous()


def gram_into(P, kernel, x1, x2, out_view, ldout):
    """pls_kernel_gram through the C ABI into a strided (possibly unaligned) view."""
    L = P.pkg._lib
    a, b = cu(x1).contiguous(), cu(x2).contiguous()
    ls = kernel._lengthscale_dev(a.shape[1])
    assert ls.numel() == a.shape[1] + L.kernel_shape_params(kernel.kind, a.shape[1])
    L.check(L.load().pls_kernel_gram(kernel.kind, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], ls.data_ptr(),
                                     float(kernel.outputscale), out_view.data_ptr(), ldout, L.stream_ptr()), "pls_kernel_gram")


def grad_sums(P, kind, x, params, s, alpha, p_view, ldp):
    """pls_kernel_grad_sums through the C ABI; p_view: a device (n, n) view with leading dimension ldp"""
    L = P.pkg._lib
    lib = L.load()
    n, d = x.shape
    count = d + 1 + L.kernel_shape_params(kind, d)
    xd, ad = cu(x).contiguous(), cu(alpha).contiguous()
    nbytes = lib.pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d)
    assert nbytes > 0 and params.numel() == count - 1
    ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=F64, device="cuda")
    out = torch.full((count + 1,), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_grad_sums(kind, xd.data_ptr(), n, d, params.data_ptr(), float(s), ad.data_ptr(), p_view.data_ptr(), ldp,
                                     out.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "pls_kernel_grad_sums")
    host = out.cpu()
    assert torch.isnan(host[count]) and torch.isnan(ws[-1]).item(), f"the reduction wrote past its {count} outputs or its workspace"
    return host[:count]


def p_views(p):
    """(even ldp on a 16-byte boundary), (odd ldp, 8 bytes off): the two load paths"""
    n = p.shape[0]
    ldp = (n + 1) // 2 * 2
    buf = torch.full((n, ldp), float("nan"), dtype=F64, device="cuda")
    buf[:, :n] = cu(p)
    ldo = n + 1 + (n % 2)
    raw = torch.full((1 + n * ldo,), float("nan"), dtype=F64, device="cuda")
    view = raw[1:].view(n, ldo)
    view[:, :n] = cu(p)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and ldo % 2 == 1
    return (buf, ldp), (view, ldo)


def gp_mll(P, kind, x, y, params, s, noise, mean, jitter=0.0, fill=None):
    """pls_gp_mll_grad through the C ABI: (the 4 + d + shape parameters outputs on the CPU, info, status)"""
    L = P.pkg._lib
    lib = L.load()
    n, d = x.shape
    width = 4 + d + L.kernel_shape_params(kind, d)
    assert params.numel() == width - 4
    xd, yd = cu(x).contiguous(), cu(y).contiguous()
    nbytes = lib.pls_gp_mll_workspace_bytes_kind(kind, n, d)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    out = torch.full((width + 1,), float("nan"), dtype=F64, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = lib.pls_gp_mll_grad(kind, xd.data_ptr(), n, d, params.data_ptr(), float(s), float(noise), float(mean), float(jitter),
                             yd.data_ptr(), out.data_ptr(), info.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr())
    host = out.cpu()
    assert torch.isnan(host[width]), f"the evaluation wrote past its {width} outputs"
    return host[:width], int(info.item()), rc


def kernel_mean(P, kind, xd, params, ad, xtd, s, mean):
    """pls_kernel_mean through the C ABI on device operands as given (their alignment is part of the tests)"""
    L = P.pkg._lib
    (n, d), t = xd.shape, xtd.shape[0]
    assert params.numel() == d + L.kernel_shape_params(kind, d)
    out = torch.full((t + 1,), float("nan"), dtype=F64, device="cuda")
    L.check(L.load().pls_kernel_mean(kind, xd.data_ptr(), n, d, params.data_ptr(), float(s), float(mean), ad.data_ptr(), xtd.data_ptr(), t,
                                     out.data_ptr(), L.stream_ptr()), "pls_kernel_mean")
    host = out.cpu()
    assert torch.isnan(host[t]), "pls_kernel_mean wrote past its t outputs"
    return host[:t]


def offset_copy(m):
    """a contiguous device copy of m that starts 8 bytes past a 16-byte boundary, a NaN in front"""
    raw = torch.full((1 + m.numel(),), float("nan"), dtype=F64, device="cuda")
    view = raw[1:].view(m.shape)
    view.copy_(m)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view
