"""What one epoch of Dirichlet exact-GP classification costs on the library, and what the class probabilities cost.

    python tools/dirichlet_gp_probe.py [--out profiles/dirichlet_gp.txt] [--sizes 500 2000] [--classes 2] [--repeats 20]

1. Per epoch: ONE pls_gp_mll_grad_classes call for all C classes with its one read-back, beside C calls of pls_gp_mll_grad
   with a read-back each (what a caller without the new entry would do; that entry has no per-point noise, so its matrix
   lacks the fixed part -- the work is the same).  Host clock from the first launch to the end of the last read-back (a
   device-to-host copy synchronises), the two variants alternating, median and range of the repeats after a warm-up.
2. DirichletExactGP.predict_proba at t = 2000 test points and S = 256 samples: the whole call (host clock, ends in a
   read-back) and pls_softmax_normal_mean alone (device events around 200 back-to-back launches, per launch).
Needs the MI355X; there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import projected_langevin_sampling_amd as pkg  # noqa: E402

L = pkg._lib
F64 = torch.float64
KERNEL_BATCH = 200  # launches of the probability kernel between two events: one launch is far below the events' resolution


def spread(ms):
    return f"{statistics.median(ms):9.3f} {min(ms):9.3f} {max(ms):9.3f}"


def epoch_times(n, d, classes, repeats):
    lib = L.load()
    g = torch.Generator().manual_seed(n + classes)
    x = torch.randn(n, d, generator=g, dtype=F64)
    labels = (torch.sin(1.5 * x[:, 0]) + 0.5 * x[:, -1] > 0).long() if classes == 2 else torch.randint(0, classes, (n,), generator=g)
    model = pkg.DirichletExactGP(x, labels, "rbf", number_of_classes=classes)
    st = model._device_state()
    ls = st["x"].new_tensor(model.lengthscale.tolist())
    s, noise, mean = model.outputscale.tolist(), model.noise.tolist(), model.mean_constant.tolist()
    nbytes = lib.pls_gp_mll_workspace_bytes(n, d)
    single = torch.zeros(4 + d + 1, dtype=F64, device="cuda")

    host = [(ctypes.c_double * classes)(*v) for v in (s, noise, mean)]
    hp = [ctypes.cast(a, ctypes.c_void_p) for a in host]
    width = 4 + d

    def one_call():  # (both variants call the C ABI directly with prepared arguments: the same host work per call)
        L.check(lib.pls_gp_mll_grad_classes(model.kind, st["x"].data_ptr(), n, d, classes, ls.data_ptr(), hp[0], hp[1], hp[2],
                                            st["fixed"].data_ptr(), n, st["y"].data_ptr(), n, 0.0, st["out"].data_ptr(),
                                            st["out"].data_ptr() + 8 * classes * width, st["ws"].data_ptr(), nbytes,
                                            L.stream_ptr()), "pls_gp_mll_grad_classes")
        got = st["out"].cpu()
        assert not got[classes * width:].view(torch.int32)[:classes].any()
        return got

    def per_class_calls():
        rows = []
        for c in range(classes):
            L.check(lib.pls_gp_mll_grad(model.kind, st["x"].data_ptr(), n, d, ls[c].data_ptr(), s[c], noise[c], mean[c], 0.0,
                                        st["y"][c].data_ptr(), single.data_ptr(), single.data_ptr() + 8 * (4 + d),
                                        st["ws"].data_ptr(), nbytes, L.stream_ptr()), "pls_gp_mll_grad")
            rows.append(single.cpu())
        return rows

    for fn in (one_call, per_class_calls):
        fn()
    torch.cuda.synchronize()
    t_one, t_per = [], []
    for _ in range(repeats):
        for fn, sink in ((one_call, t_one), (per_class_calls, t_per)):
            t0 = time.perf_counter()
            fn()
            sink.append(1e3 * (time.perf_counter() - t0))
    return t_one, t_per


def proba_times(n, d, classes, t, samples, repeats):
    g = torch.Generator().manual_seed(t)
    x = torch.randn(n, d, generator=g, dtype=F64)
    labels = torch.randint(0, classes, (n,), generator=g)
    model = pkg.DirichletExactGP(x, labels, "rbf", number_of_classes=classes)
    xt = torch.randn(t, d, generator=g, dtype=F64).cuda()
    mean, var = model.predict(xt)
    model.predict_proba(xt, samples).cpu()
    torch.cuda.synchronize()
    whole, kernel = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.predict_proba(xt, samples).cpu()
        whole.append(1e3 * (time.perf_counter() - t0))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(KERNEL_BATCH):
            pkg.softmax_normal_mean(mean, var, samples)
        b.record()
        b.synchronize()
        kernel.append(a.elapsed_time(b) / KERNEL_BATCH)
    return whole, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dirichlet_gp.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    c, d = args.classes, 2
    lines = [f"# tools/dirichlet_gp_probe.py on {torch.cuda.get_device_name(0)}: milliseconds, median / min / max of {args.repeats} after a warm-up",
             f"# 1. one epoch's evaluation of C = {c} classes, d = {d}, RBF: host clock from the first launch to the end of the last read-back",
             f"{'n':>5s} {'variant':42s} {'median':>9s} {'min':>9s} {'max':>9s}"]
    for n in args.sizes:
        t_one, t_per = epoch_times(n, d, c, args.repeats)
        lines.append(f"{n:5d} {'1 classes call, 1 read-back':42s} {spread(t_one)}")
        lines.append(f"{n:5d} {f'{c} pls_gp_mll_grad calls, {c} read-backs':42s} {spread(t_per)}")
        print("\n".join(lines[-2:]), flush=True)
    t, samples, n = 2000, 256, args.sizes[0]
    whole, kernel = proba_times(n, d, c, t, samples, args.repeats)
    lines += [f"# 2. class probabilities at t = {t} test points, S = {samples} samples, C = {c}, n = {n}",
              f"{'':5s} {'predict_proba (host clock)':42s} {spread(whole)}",
              f"{'':5s} {f'pls_softmax_normal_mean (events, per launch of {KERNEL_BATCH})':42s} {spread(kernel)}"]
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
