"""GPU: every 32-bit byte-offset path of the kernels at its leading-dimension limit (profiles/large_ld_limits.txt).

The MFMA kernels address operands with 32-bit byte offsets behind 2 GiB buffer descriptors while every entry takes its
leading dimensions as int64.  Past a limit a range-checked load returns zeros and a range-checked store is dropped: a wrong
answer, not an error.  Each case here puts ONE operand at a leading dimension next to a limit of the table -- the last value
a path takes, the first one the next path takes, the last one an entry accepts and one it must refuse -- and asserts one of
three outcomes: the exact result (integer operands: torch.equal with plain fp64 torch on the host) inside an intact sentinel
arena (tests/large_ld.py), a refusal that names the leading dimension, or the exact result of the path the call is routed to
(the route asserted where the library reports it).  Wrong-but-finite output is what these tests exist to catch."""
import contextlib
import copy

import pytest
import torch

from large_ld import (DIRECT_MAX_LD, KSPLIT_MAX_LD, SMALL_RANK_MAX_LD, Budget, gemm_dma_max_ld, gemm_route, ints, ipb_prep_max_ld,
                      refused, strip_max_ld)
from step_fixtures import EXACT_ETA, ExactProblem, exact_ipb, option
from test_gpu_exact_ipb import factor
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PAST = 2 ** 16  # how far past a limit the refused / routed cases sit


def past(limit):
    """the issue's L + 2^16, made even where the limit is odd (an odd stride takes the scalar-load path, a case of its own)"""
    return (limit + PAST + 1) & ~1


def even_below(limit):
    """the issue's L - 2 for an even limit; the largest even value below an odd one (the DMA paths need even strides)"""
    return (limit - 2) & ~1 if limit % 2 == 0 else limit - 1


# -------------------------------------------------------------------------------------------------------------------------
# pls_gemm_tn: K = 35 is two 16-row DMA steps plus a 3-row tail (one k-split super-step of 32 rows plus a tail)
K = 35
GEMM_CONFIGS = {  # name: (I, J, PLS_OPT_KSPLIT_MODE); the name is the route at ordinary strides
    "tiles_128": (128, 32768, 1),   # 256 tiles of 128 x 128: LDS-DMA k-loop
    "tiles_64": (128, 128, 0),
    "ksplit_1": (128, 128, 3),
    "ksplit_2": (128, 128, 2),
    "row_blocks": (144, 16384, 1),  # 2 x 128 tiles of 80 rows (gemm_rows_ok), LDS-DMA k-loop
}
DMA_CONFIGS = ("tiles_128", "row_blocks")


def gemm_cases():
    cases = []
    for cfg, (i, j, _) in GEMM_CONFIGS.items():
        for ld in (DIRECT_MAX_LD - 2, DIRECT_MAX_LD, DIRECT_MAX_LD + 2):  # last direct store, first and second LDS-epilogue stores
            cases.append((cfg, "c", ld, 0))
        for op, cols in (("l", i), ("r", j)):
            for ld in (KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD):  # last k-split launch, first one handed to the tile kernels
                cases.append((cfg, op, ld, 0))
            lim = gemm_dma_max_ld(cols)
            cases.append((cfg, op, even_below(lim), 0))
            cases.append((cfg, op, past(lim), 0))  # DMA configurations: refused; the others have no limit
    # the limit itself, and the scalar-load path (odd stride; a view 8 bytes off a 16-byte boundary), which has no limit
    cases.append(("tiles_128", "l", gemm_dma_max_ld(128), 0))
    cases.append(("tiles_128", "r", past(gemm_dma_max_ld(32768)) + 1, 0))
    cases.append(("tiles_128", "l", past(gemm_dma_max_ld(128)), 1))
    return cases


_gemm_inputs = {}


def gemm_inputs(i, j):
    if (i, j) not in _gemm_inputs:
        l, r = ints((K, i), 7, 11 + i), ints((K, j), 7, 13 + j)
        _gemm_inputs[(i, j)] = (l, r, l.T @ r)  # |sums| <= 35 * 49: exact in any order
    return _gemm_inputs[(i, j)]


@pytest.mark.parametrize("cfg,operand,ld,lead", gemm_cases(), ids=lambda v: str(v))
def test_gemm_tn(P, cfg, operand, ld, lead):
    L, lib = P.pkg._lib, P.pkg._lib.load()
    i, j, mode = GEMM_CONFIGS[cfg]
    l, r, want = gemm_inputs(i, j)
    ldl, ldr, ldc = (ld if operand == "l" else i + 16), (ld if operand == "r" else j + 16), (ld if operand == "c" else j + 16)
    vec = ldl % 2 == 0 and ldr % 2 == 0 and lead % 2 == 0
    refuse = cfg in DMA_CONFIGS and vec and (ldl > gemm_dma_max_ld(i) or ldr > gemm_dma_max_ld(j))
    # the route the table predicts: k-split below 2^22 only, row blocks below 2^21 (ldc) only
    route = cfg
    if cfg.startswith("ksplit") and max(ldl, ldr) >= KSPLIT_MAX_LD:
        route = "tiles_64"
    if cfg == "row_blocks" and ldc >= DIRECT_MAX_LD:
        route = "tiles_128"
    with Budget() as b, ksplit(P, mode):
        al = b.arena(K, i, ldl, lead if operand == "l" else 0, l)
        ar = b.arena(K, j, ldr, lead if operand == "r" else 0, r)
        ac = b.arena(i, j, ldc)
        got_route, direct = gemm_route(L, lib, al.ptr, ldl, ar.ptr, ldr, ldc, i, j, K)
        rc = lib.pls_gemm_tn(al.ptr, ldl, ar.ptr, ldr, ac.ptr, ldc, i, j, K, 1.0, 0.0, L.stream_ptr())
        torch.cuda.synchronize()
        what = f"{cfg} ld{operand}={ld} lead={lead}"
        if refuse:
            if rc == 0:  # not refused: report what the kernel made of the stride, then fail for the missing refusal
                ac.check(want, what + " (the call was not refused)")
            refused(lib, rc, f"ld{operand}={ld}")
            assert got_route is None, f"{what}: pls_gemm_tn_route reports {got_route} for a refused call"
            ac.check("untouched", what)
        else:
            L.check(rc, what)
            assert got_route == route, f"{what}: routed to {got_route}, the table says {route}"
            assert direct == (1 if ldc < DIRECT_MAX_LD else 0), f"{what}: direct_store {direct}"
            ac.check(want, what)
        al.check(what=what + " (L)")
        ar.check(what=what + " (R)")


# -------------------------------------------------------------------------------------------------------------------------
# the solves: m = 128 (one block row) and 257 (three, the last of one row); j = 96 is three strips, 80 leaves the last ragged
def solve_calls(P, f, m, jj, au, av, mode):
    """(name, substitutes, call) of every solve entry under PLS_OPT_SOLVE_MODE ``mode``"""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    d = f.desc()
    ws = torch.empty(m * jj, device="cuda")
    st = L.stream_ptr()
    return [
        ("pls_chol_solve", True, "v", lambda: lib.pls_chol_solve(d, au.ptr, au.ld, jj, av.ptr, av.ld, st)),
        ("pls_chol_forward_solve", mode == 0, "s", lambda: lib.pls_chol_forward_solve(d, au.ptr, au.ld, jj, av.ptr, av.ld, st)),
        ("pls_chol_solve_ws", mode == 0, "v",
         lambda: lib.pls_chol_solve_ws(d, au.ptr, au.ld, jj, av.ptr, av.ld, ws.data_ptr(), ws.numel() * 8, st)),
    ]


@pytest.mark.parametrize("over", [False, True], ids=["below", "past"])
@pytest.mark.parametrize("which", ["ldu", "ldv"])
@pytest.mark.parametrize("m", [128, 257])
def test_solves(P, m, which, over):
    """pls_chol_solve, pls_chol_forward_solve, pls_chol_solve_ws with the right-hand side or the solution at the substitution
    kernel's limit: exact below it; past it refused where the entry substitutes, exact where it multiplies (the product
    route's 64 x 64 tiles and k-split kernels load through 64-bit pointers or are routed by 2^22)."""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    ex = exact_ipb(m, 16, 96)
    f = factor(P, ex)
    want = {"v": ex.solve(ex.u), "s": ex.s}
    for jj in (96, 80):
        lim = strip_max_ld(m, jj)
        ld = past(lim) if over else even_below(lim)
        ldu, ldv = (ld, jj + 16) if which == "ldu" else (jj + 16, ld)
        with Budget() as b:
            au, av = b.arena(m, jj, ldu), b.arena(m, jj, ldv)
            for mode in (0, 1):
                with option(P, L.OPT_SOLVE_MODE, mode):
                    for name, substitutes, key, call in solve_calls(P, f, m, jj, au, av, mode):
                        what = f"{name} mode {mode} m={m} j={jj} {which}={ld}"
                        au.view.copy_(ex.u[:, :jj])
                        au.values = ex.u[:, :jj]
                        rc = call()
                        torch.cuda.synchronize()
                        if over and substitutes:
                            if rc == 0:  # not refused: report what the kernel made of the stride first
                                av.check(want[key][:, :jj], what + " (the call was not refused)")
                            refused(lib, rc, f"{which}={ld}")
                            f.reset_tri_scratch()
                            av.check("untouched", what)
                        else:
                            L.check(rc, what)
                            av.check(want[key][:, :jj], what)
                        au.check(what=what + " (U)")


@pytest.mark.parametrize("which", ["ldx", "ldo"])
@pytest.mark.parametrize("m", [128, 257])
def test_tri_multiply(P, m, which):
    """pls_tri_multiply (triangular operand 1; balanced pairing has no scratch here) and the product solves (operands 1 and 2,
    balanced pairing on and off) at the k-split routing limit 2^22 - 2 / 2^22 and far past it: no limit, exact"""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    ex = exact_ipb(m, 16, 96)
    f = factor(P, ex)
    d = f.desc()
    ws = torch.empty(m * 96, device="cuda")
    for ld in (KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD, past(strip_max_ld(m, 96))):
        ldx, ldo = (ld, 112) if which == "ldx" else (112, ld)
        with Budget() as b:
            ax, ao = b.arena(m, 96, ldx), b.arena(m, 96, ldo)
            for bal in (1, 0):
                with option(P, L.OPT_TRI_BALANCE, bal), option(P, L.OPT_SOLVE_MODE, 1):
                    for name, src, want, call in (
                        ("pls_tri_multiply", ex.xi, ex.e,
                         lambda: lib.pls_tri_multiply(f.LcT.data_ptr(), L.ld(f.LcT), m, ax.ptr, ldx, 96, ao.ptr, ldo, L.stream_ptr())),
                        ("pls_chol_solve_ws", ex.u, ex.solve(ex.u),
                         lambda: lib.pls_chol_solve_ws(d, ax.ptr, ldx, 96, ao.ptr, ldo, ws.data_ptr(), ws.numel() * 8, L.stream_ptr())),
                    ):
                        what = f"{name} balance {bal} m={m} {which}={ld}"
                        ax.view.copy_(src)
                        ax.values = src
                        L.check(call(), what)
                        torch.cuda.synchronize()
                        ao.check(want, what)
                        ax.check(what=what + " (X)")


def restrided(b, t, ld):
    """a copy of the device matrix ``t`` with leading dimension ``ld`` inside an arena of the budget ``b``"""
    return b.arena(t.shape[0], t.shape[1], ld, 0, t.cpu())


@pytest.mark.parametrize("over", [False, True], ids=["below", "past"])
def test_substitution_operators_at_their_limit(P, over):
    """ldsf / ldsb of pls_chol_desc (m = 128: a block row of each, 2 GiB apiece): exact below the limit, refused past it"""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    m, jj = 128, 96
    ex = exact_ipb(m, 16, jj)
    f = factor(P, ex)
    lim = strip_max_ld(m, m)
    ld = past(lim) if over else even_below(lim)
    with Budget() as b:
        g = copy.copy(f)
        asf, asb = restrided(b, f.Sf, ld), restrided(b, f.Sb, ld)
        g.Sf, g.Sb = asf.view, asb.view
        au, av = b.arena(m, jj, jj + 16, 0, ex.u), b.arena(m, jj, jj + 16)
        rc = lib.pls_chol_solve(g.desc(), au.ptr, au.ld, jj, av.ptr, av.ld, L.stream_ptr())
        torch.cuda.synchronize()
        what = f"pls_chol_solve ldsf=ldsb={ld}"
        if over:
            if rc == 0:
                av.check(ex.solve(ex.u), what + " (the call was not refused)")
            refused(lib, rc, f"ldsf={ld}")
            av.check("untouched", what)
        else:
            L.check(rc, what)
            av.check(ex.solve(ex.u), what)
        for a in (asf, asb, au):
            a.check(what=what)


# -------------------------------------------------------------------------------------------------------------------------
# the step routes of the orthonormal basis: M_k = 128, N = 256, J = 256, Gaussian cost, injected integer noise
ONB_ROUTES = {  # name: (force_generic, PLS_OPT_SMALL_RANK_STEP, PLS_OPT_SMALL_RANK_MAX)
    "fast": (False, 1, 128),         # B U on the k-split kernel with the Langevin update in its epilogue
    "one_launch": (True, 2, 128),    # csrc/small_rank_step.h
    "slab_kernels": (True, 0, 128),  # csrc/small_rank.h + the update launch
    "contractions": (True, 0, 0),    # forward and back-projection contractions + the update launch
}
_onb = {}


def onb_problem(P, mk, n, j):
    if (mk, n, j) not in _onb:
        ex = ExactProblem(mk, n, j, seed=mk + n + j)
        _onb[(mk, n, j)] = (ex, ex.basis(P), ex.cost(P))
    return _onb[(mk, n, j)]


def run_onb_step(P, ex, gb, cost, route, au, ao, what):
    """one step with the energies of its input particles in the same call, into the arena ``ao``; both checked"""
    L = P.pkg._lib
    generic, sr_step, sr_max = ONB_ROUTES[route]
    xi = P.basis.NoiseSpec(injected=ex.xi.cuda())
    e = torch.full((ex.j,), float("nan"), device="cuda")
    with option(P, L.OPT_SMALL_RANK_STEP, sr_step), option(P, L.OPT_SMALL_RANK_MAX, sr_max):
        gb.fused_step(cost, au.view, EXACT_ETA, noise=xi, force_generic=generic, out=ao.view, input_energy=e)
    torch.cuda.synchronize()
    want, e_want = ex.step()
    ao.check(want, what)
    au.check(what=what + " (U)")
    rel = ((e.cpu() - e_want).abs() / e_want.abs()).max().item()
    assert rel <= 1e-13, f"{what}: energy by-product, relative error {rel:.2e}"
    if hasattr(gb, "zero_step_sync"):
        gb.zero_step_sync()


@pytest.mark.parametrize("ld", [DIRECT_MAX_LD - 2, DIRECT_MAX_LD, KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["ldu", "ldo"])
@pytest.mark.parametrize("route", list(ONB_ROUTES))
def test_onb_step_routes(P, route, which, ld):
    """pls_onb_step with the particles or the output at 2^21 - 2 / 2^21 (the Langevin epilogue's direct store, which reads U
    and writes the output with one descriptor each) and 2^22 - 2 / 2^22 (the particles as an operand of the k-split
    contraction): exact on every route"""
    mk, n, j = 128, 256, 256
    ex, gb, cost = onb_problem(P, mk, n, j)
    with Budget() as b:
        au = b.arena(mk, j, ld if which == "ldu" else j + 16, 0, ex.u)
        ao = b.arena(mk, j, ld if which == "ldo" else j + 16)
        run_onb_step(P, ex, gb, cost, route, au, ao, f"onb step {route} {which}={ld}")


@pytest.mark.parametrize("ld", [DIRECT_MAX_LD - 2, DIRECT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["ldu", "ldo"])
def test_onb_fast_path_on_the_big_tiles(P, which, ld):
    """M_k = 128, J = 32768: 256 tiles of 128 x 128, whose interior tiles run the whole Langevin update in the MFMA register
    layout below 2^21 (EpiLangevinGaussian::apply_direct) and through LDS from 2^21 on"""
    mk, n, j = 128, 64, 32768
    ex, gb, cost = onb_problem(P, mk, n, j)
    with Budget() as b:
        au = b.arena(mk, j, ld if which == "ldu" else j + 16, 0, ex.u)
        ao = b.arena(mk, j, ld if which == "ldo" else j + 16)
        run_onb_step(P, ex, gb, cost, "fast", au, ao, f"onb fast path, big tiles, {which}={ld}")


@pytest.mark.parametrize("ld", [DIRECT_MAX_LD, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["ldu", "ldo"])
@pytest.mark.parametrize("route", ["one_launch", "slab_kernels", "contractions"])
def test_onb_generic_routes_with_a_bernoulli_cost(P, route, which, ld):
    """A cost without the Gaussian algebra (Bernoulli / sigmoid) on the three generic routes.  Its values are not dyadic, so
    the reference is the same call at ordinary strides (tests/test_gpu_cost_routes.py holds that to the truth): a stride
    changes no operation and no summation order, so the strided step and its energies must be the same bits."""
    L = P.pkg._lib
    mk, n, j = 128, 256, 256
    ex, gb, _ = onb_problem(P, mk, n, j)
    cost = P.costs.BernoulliCost((ex.y > 0).double(), P.links.SigmoidLinkFunction())
    generic, sr_step, sr_max = ONB_ROUTES[route]
    xi = P.basis.NoiseSpec(injected=ex.xi.cuda())

    def step(u, out):
        e = torch.full((j,), float("nan"), device="cuda")
        with option(P, L.OPT_SMALL_RANK_STEP, sr_step), option(P, L.OPT_SMALL_RANK_MAX, sr_max):
            gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=generic, out=out, input_energy=e)
        torch.cuda.synchronize()
        gb.zero_step_sync()
        return e.cpu()

    plain = torch.empty(mk, j, device="cuda")
    e_want = step(ex.u.cuda(), plain)
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    with Budget() as b:
        au = b.arena(mk, j, ld if which == "ldu" else j + 16, 0, ex.u)
        ao = b.arena(mk, j, ld if which == "ldo" else j + 16)
        e = step(au.view, ao.view)
        what = f"onb step {route}, Bernoulli cost, {which}={ld}"
        ao.check(plain.cpu(), what)
        au.check(what=what + " (U)")
        assert torch.equal(e, e_want), f"{what}: energies"


def with_operand(gb, b, name, ld):
    """a copy of the basis whose descriptor carries the matrix ``name`` with leading dimension ``ld`` (inside an arena)"""
    g = copy.copy(gb)
    g.__dict__.pop("_desc_cache", None)
    a = restrided(b, getattr(gb, name), ld)
    setattr(g, name, a.view)
    return g, a


@pytest.mark.parametrize("ld", [SMALL_RANK_MAX_LD, past(SMALL_RANK_MAX_LD)], ids=lambda v: str(v))
@pytest.mark.parametrize("route", ["one_launch", "slab_kernels"])
def test_small_rank_operand_at_its_limit(P, route, ld):
    """ldat at the fused small-rank kernels' limit (N = 64 keeps At inside 4.3 GB): the last leading dimension they take, and
    one past it, where the step is routed to the contraction kernels -- exact either way"""
    mk, n, j = 128, 64, 256
    ex, gb, cost = onb_problem(P, mk, n, j)
    with Budget() as b:
        g, aat = with_operand(gb, b, "_At", ld)
        au, ao = b.arena(mk, j, j + 16, 0, ex.u), b.arena(mk, j, j + 16)
        with P.pkg._lib.Timeline(64) as tl:
            run_onb_step(P, ex, g, cost, route, au, ao, f"onb step {route} ldat={ld}")
        tag = "small_rank_step" if route == "one_launch" else "small_rank_drift"
        assert (tag in tl.summary()) == (ld <= SMALL_RANK_MAX_LD), f"ldat={ld}: launches {sorted(tl.summary())}"
        aat.check(what=f"ldat={ld} (At)")


@pytest.mark.parametrize("ld", [KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["_A", "_At", "_B"])
def test_onb_descriptor_operands_on_the_contractions(P, name, ld):
    """lda / ldat at the k-split routing limit on the general route's contractions, ldb on the Gaussian fast path's"""
    mk, n, j = 128, 256, 256
    ex, gb, cost = onb_problem(P, mk, n, j)
    gb.prepare_gaussian(cost.y_device())
    route = "fast" if name == "_B" else "contractions"
    with Budget() as b:
        g, a = with_operand(gb, b, name, ld)
        au, ao = b.arena(mk, j, j + 16, 0, ex.u), b.arena(mk, j, j + 16)
        run_onb_step(P, ex, g, cost, route, au, ao, f"onb step {route} {name} ld={ld}")
        a.check(what=f"{name} ld={ld}")


# -------------------------------------------------------------------------------------------------------------------------
# forward map and the element-wise cost entries: 64-bit indexing, no limit
@pytest.mark.parametrize("ld", [DIRECT_MAX_LD - 2, DIRECT_MAX_LD, KSPLIT_MAX_LD + 2], ids=lambda v: str(v))
def test_forward_and_cost_entries(P, ld):
    """pls_onb_forward into F, pls_cost_derivative from F into G, pls_cost_value from F, each strided operand on its own"""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    mk, n, j = 128, 256, 256
    ex, gb, cost = onb_problem(P, mk, n, j)
    f_want = ex.a.T @ ex.u
    g_want = (f_want - ex.y[:, None]) / 0.25
    c_want = ((f_want - ex.y[:, None]) ** 2).sum(0) / 0.5
    st = L.stream_ptr()
    with Budget() as b:
        au, af = b.arena(mk, j, j + 16, 0, ex.u), b.arena(n, j, ld)
        L.check(lib.pls_onb_forward(gb._desc(), au.ptr, au.ld, j, af.ptr, ld, st), "pls_onb_forward")
        torch.cuda.synchronize()
        af.check(f_want, f"pls_onb_forward ldf={ld}")
        au.check(what="pls_onb_forward (U)")
    with Budget() as b:
        au, af = b.arena(mk, j, ld, 0, ex.u), b.arena(n, j, j + 16)
        L.check(lib.pls_onb_forward(gb._desc(), au.ptr, ld, j, af.ptr, af.ld, st), "pls_onb_forward")
        torch.cuda.synchronize()
        af.check(f_want, f"pls_onb_forward ldu={ld}")
        au.check(what="pls_onb_forward (U)")
    y = cost.y_device()
    for ldf, ldg in ((ld, j + 16), (j + 16, ld)):
        with Budget() as b:
            af, ag = b.arena(n, j, ldf, 0, f_want), b.arena(n, j, ldg)
            L.check(lib.pls_cost_derivative(cost.desc(), af.ptr, ldf, y.data_ptr(), n, j, ag.ptr, ldg, st), "pls_cost_derivative")
            torch.cuda.synchronize()
            ag.check(g_want, f"pls_cost_derivative ldf={ldf} ldg={ldg}")
            af.check(what="pls_cost_derivative (F)")
    with Budget() as b:
        af = b.arena(n, j, ld, 0, f_want)
        c = torch.empty(j, device="cuda")
        nb = lib.pls_cost_value_workspace_bytes(n, j)
        ws = torch.empty(nb // 8 + 1, device="cuda")
        L.check(lib.pls_cost_value(cost.desc(), af.ptr, ld, y.data_ptr(), n, j, c.data_ptr(), ws.data_ptr(), nb, st), "pls_cost_value")
        torch.cuda.synchronize()
        assert torch.equal(c.cpu(), c_want), f"pls_cost_value ldf={ld}"
        af.check(what="pls_cost_value (F)")


# -------------------------------------------------------------------------------------------------------------------------
# the inducing-point basis: M = 128, N = 256, J = 256
_ipb = {}


def ipb_problem(P, m, n, j, fast=False):
    """(problem, basis, cost) with the Gaussian operators built; ``fast``: a basis outside whitened coordinates that also
    carries the explicit inverse W (the B V route, and W U under PLS_OPT_IPB_EXPLICIT_INVERSE)"""
    if (m, n, j, fast) not in _ipb:
        ex = exact_ipb(m, n, j)
        gb, cost = ex.basis(P, explicit_inverse=fast), ex.cost(P)
        if fast:
            gb.whitened = False
        gb._prepare_for(cost)
        _ipb[(m, n, j, fast)] = (ex, gb, cost)
    return _ipb[(m, n, j, fast)]


def run_ipb_step(P, ex, gb, cost, generic, au, ao, what, whitened=False, opts=None, energy=True):
    """one step into the arena ``ao`` under the route options ``opts`` (default: the one-launch step wherever it applies), with
    the energies of the input particles in the same call unless ``energy`` is False; all checked"""
    L = P.pkg._lib
    xi = P.basis.NoiseSpec(injected=(ex.xi if whitened else ex.injected).cuda())
    e = torch.full((ex.j,), float("nan"), device="cuda") if energy else None
    entry = gb.whitened_step if whitened else gb.fused_step
    with contextlib.ExitStack() as stack:
        for opt, mode in ({L.OPT_SMALL_RANK_STEP: 2} if opts is None else opts).items():
            stack.enter_context(option(P, opt, mode))
        entry(cost, au.view, EXACT_ETA, noise=xi, force_generic=generic, out=ao.view, input_energy=e)
    torch.cuda.synchronize()
    want, e_want = ex.whitened_step() if whitened else ex.step()
    ao.check(want, what)
    au.check(what=what + " (particles)")
    if energy:
        rel = ((e.cpu() - e_want).abs() / e_want.abs()).max().item()
        assert rel <= 1e-13, f"{what}: energy by-product, relative error {rel:.2e}"
    if hasattr(gb, "zero_step_sync"):
        gb.zero_step_sync()


@pytest.mark.parametrize("ld", [DIRECT_MAX_LD - 2, DIRECT_MAX_LD, KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["ldu", "ldo"])
@pytest.mark.parametrize("entry", ["gaussian", "generic", "whitened"])
def test_ipb_step_routes(P, entry, which, ld):
    """pls_ipb_step on the Gaussian route of a whitened basis and on the one-launch route (solve-and-noise launch + small-rank step), and
    pls_ipb_whitened_step, with the particles or the output strided"""
    m, n, j = 128, 256, 256
    ex, gb, cost = ipb_problem(P, m, n, j)
    whitened = entry == "whitened"
    with Budget() as b:
        au = b.arena(m, j, ld if which == "ldu" else j + 16, 0, ex.s if whitened else ex.u)
        ao = b.arena(m, j, ld if which == "ldo" else j + 16)
        run_ipb_step(P, ex, gb, cost, entry == "generic", au, ao, f"ipb step {entry} {which}={ld}", whitened)


@pytest.mark.parametrize("over", [False, True], ids=["below", "past"])
def test_solve_and_noise_launch_at_its_limit(P, over):
    """ldlinv / ldlinvt at the limit of csrc/ipb_prep.hip: the last even leading dimension its descriptor spans, and one past
    it, where the step is routed to the separate solve launches -- exact either way"""
    m, n, j = 128, 256, 256
    ex, gb, cost = ipb_problem(P, m, n, j)
    lim = ipb_prep_max_ld(m)
    ld = past(lim) if over else even_below(lim)
    with Budget() as b:
        g = copy.copy(gb)
        g.__dict__.pop("_desc_cache", None)
        g._chol = copy.copy(gb._chol)
        ali, alt = restrided(b, gb._chol.Linv, ld), restrided(b, gb._chol.LinvT, ld)
        g._chol.Linv, g._chol.LinvT = ali.view, alt.view
        au, ao = b.arena(m, j, j + 16, 0, ex.u), b.arena(m, j, j + 16)
        with P.pkg._lib.Timeline(64) as tl:
            run_ipb_step(P, ex, g, cost, True, au, ao, f"ipb one-launch route ldlinv=ldlinvt={ld}")
        assert ("ipb_prep" in tl.summary()) == (not over), f"ld={ld}: launches {sorted(tl.summary())}"
        ali.check(what="Linv")
        alt.check(what="LinvT")


def ipb_with_operand(gb, b, attr, ld):
    """a copy of the inducing-point basis whose descriptor carries the matrix ``attr`` (``LcT``: of its factor) with leading
    dimension ``ld`` inside an arena"""
    g = copy.copy(gb)
    if attr == "LcT":
        g._chol = copy.copy(gb._chol)
        a = restrided(b, gb._chol.LcT, ld)
        g._chol.LcT = a.view
    else:
        a = restrided(b, getattr(gb, attr), ld)
        setattr(g, attr, a.view)
    return g, a


def ipb_operand_routes(L):
    """descriptor field: (attribute, N, fast basis, force_generic, route options, energies asked for, what reads the operand)"""
    contractions = {L.OPT_SMALL_RANK_STEP: 0, L.OPT_SMALL_RANK_MAX: 0}
    return {
        "ldkzx": ("base_gram_induce_train", 256, False, True, contractions, True, "general route: F = k(X,Z) V"),
        "ldkxz": ("_Kxz", 64, False, True, contractions, True, "general route: k(Z,X) G"),
        "ldw": ("_W", 256, True, True, {**contractions, L.OPT_IPB_EXPLICIT_INVERSE: 1}, True, "general route: V = W U"),
        "ldb": ("_B", 256, True, False, {}, True, "Gaussian route outside whitened coordinates: B V"),
        "ldq": ("_Q", 256, False, False, {}, True, "whitened route with energies: Q S in the fused kernel"),
        "ldpt": ("_Pt", 256, False, False, {}, False, "whitened route: P U in the fused kernel"),
        "ldlct": ("LcT", 256, False, False, {}, False, "whitened route: Lc dS (triangular operand 1)"),
    }


@pytest.mark.parametrize("ld", [KSPLIT_MAX_LD - 2, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("field", ["ldkzx", "ldkxz", "ldw", "ldb", "ldq", "ldpt", "ldlct"])
def test_ipb_descriptor_operands_on_the_contractions(P, field, ld):
    """Every M x M or M x N operand of pls_ipb_desc on the route whose contraction reads it (M = 128, J = 256: fewer than 256
    tiles, so the k-split kernel below 2^22 and the 64 x 64 tiles from 2^22 on): the last k-split launch and the first one
    handed to the tile kernels, exact either way"""
    attr, n, fast, generic, opts, energy, reads = ipb_operand_routes(P.pkg._lib)[field]
    m, j = 128, 256
    ex, gb, cost = ipb_problem(P, m, n, j, fast)
    with Budget() as b:
        g, a = ipb_with_operand(gb, b, attr, ld)
        au, ao = b.arena(m, j, j + 16, 0, ex.u), b.arena(m, j, j + 16)
        what = f"ipb step, {reads}, {field}={ld}"
        run_ipb_step(P, ex, g, cost, generic, au, ao, what, opts=opts, energy=energy)
        a.check(what=what + f" ({attr})")


@pytest.mark.parametrize("ld", [SMALL_RANK_MAX_LD, past(SMALL_RANK_MAX_LD)], ids=lambda v: str(v))
@pytest.mark.parametrize("route", ["one_launch", "slab_kernels"])
def test_ipb_small_rank_operand_at_its_limit(P, route, ld):
    """ldkxz at the fused small-rank kernels' limit (N = 64 keeps k(X,Z) inside 4.3 GB): the last leading dimension the
    one-launch step and the slab kernel take, and one past it, where pls_ipb_step is routed to the contraction kernels --
    exact either way"""
    L = P.pkg._lib
    m, n, j = 128, 64, 256
    ex, gb, cost = ipb_problem(P, m, n, j)
    opts = {L.OPT_SMALL_RANK_STEP: 2} if route == "one_launch" else {L.OPT_SMALL_RANK_STEP: 0, L.OPT_SMALL_RANK_MAX: 128}
    with Budget() as b:
        g, a = ipb_with_operand(gb, b, "_Kxz", ld)
        au, ao = b.arena(m, j, j + 16, 0, ex.u), b.arena(m, j, j + 16)
        with L.Timeline(64) as tl:
            run_ipb_step(P, ex, g, cost, True, au, ao, f"ipb step {route} ldkxz={ld}", opts=opts)
        fused = sorted(t for t in tl.summary() if t.startswith("small_rank"))
        if ld <= SMALL_RANK_MAX_LD:
            assert fused and (route != "one_launch" or fused == ["small_rank_step"]), f"ldkxz={ld}: launches {sorted(tl.summary())}"
        else:
            assert not fused, f"ldkxz={ld}: launches {sorted(tl.summary())}"
        a.check(what=f"ldkxz={ld} (Kxz)")


@pytest.mark.parametrize("ld", [DIRECT_MAX_LD, KSPLIT_MAX_LD], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["lds", "ldo"])
def test_ipb_whitened_generic_step(P, which, ld):
    """pls_ipb_whitened_generic_step (M = 64, a power of four: the prior rows of Awa are exact) with the whitened particles or
    the output strided"""
    m, n, j = 64, 256, 256
    ex, gb, cost = ipb_problem(P, m, n, j)
    assert gb.whitened_generic_applies(cost, j, force_generic=True)
    with Budget() as b:
        au = b.arena(m, j, ld if which == "lds" else j + 16, 0, ex.s)
        ao = b.arena(m, j, ld if which == "ldo" else j + 16)
        run_ipb_step(P, ex, gb, cost, True, au, ao, f"ipb whitened generic step {which}={ld}", whitened=True)


@pytest.mark.parametrize("over", [False, True], ids=["at", "past"])
def test_whitened_operand_at_its_limit(P, over):
    """ldawa at the one-launch step's limit (N = 16 keeps Awa's 80 rows inside 5.4 GB): exact at 2^23; past it the entry, which
    has no other kernel to hand the operand to, refuses and pls_ipb_whitened_generic_applies says so beforehand"""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    m, n, j = 64, 16, 256
    ex, gb, cost = ipb_problem(P, m, n, j)
    assert gb.whitened_generic_applies(cost, j, force_generic=True)
    ld = past(SMALL_RANK_MAX_LD) if over else SMALL_RANK_MAX_LD
    with Budget() as b:
        g, aw = with_operand(gb, b, "_Awa", ld)
        au, ao = b.arena(m, j, j + 16, 0, ex.s), b.arena(m, j, j + 16)
        what = f"ipb whitened generic step ldawa={ld}"
        y = cost.y_device()
        assert lib.pls_ipb_whitened_generic_applies(g._desc(), y.data_ptr(), j) == (0 if over else 1), what
        if over:
            nbytes = lib.pls_ipb_whitened_generic_workspace_bytes(g._desc(), j)
            ws = torch.empty(nbytes // 8 + 1, device="cuda")
            xi = P.basis.NoiseSpec(injected=ex.xi.cuda())
            rc = lib.pls_ipb_whitened_generic_step(g._desc(), cost.desc(), y.data_ptr(), au.ptr, au.ld, j, EXACT_ETA, None, xi.desc(),
                                                   ao.ptr, ao.ld, L.OUT_DELTA, None, ws.data_ptr(), nbytes, L.stream_ptr())
            torch.cuda.synchronize()
            refused(lib, rc, f"ldawa={ld}")
            ao.check("untouched", what)
            au.check(what=what + " (S)")
        else:
            run_ipb_step(P, ex, g, cost, True, au, ao, what, whitened=True)
        aw.check(what=what + " (Awa)")
