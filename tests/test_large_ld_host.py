"""CPU: the leading-dimension limits of the kernels' 32-bit byte offsets (profiles/large_ld_limits.txt), as the host side
applies them.  Argument validation and routing happen before any launch, so the refusals and the routes are pinned without a
GPU: the limits the library reports (pls_ld_limit: the very functions its guards call) against the table's formulas, the
route of pls_gemm_tn on either side of every limit (pls_gemm_tn_route: the launchers' own predicates), and the refusal of
every entry whose kernel cannot address the stride, with a message that names the leading dimension.  A call that is NOT
refused would launch, so an entry itself is only ever called where it refuses; the other side of each limit -- ld = limit is
taken -- is asked of the predicate the entry itself calls, exported without the launch behind it: pls_gemm_tn_route,
pls_chol_solve_check, pls_small_rank_route, pls_ipb_prep_applies, pls_ipb_whitened_generic_applies; or of the entry with a
second argument it refuses AFTER the stride check (pls_ipb_whitened_generic_step), whose message then tells which fired."""
import ctypes

import pytest

from large_ld import (DIRECT_MAX_LD, KSPLIT_MAX_LD, SMALL_RANK_MAX_LD, gemm_dma_max_ld, ipb_prep_max_ld, strip_max_ld)


@pytest.fixture(scope="module")
def lib():
    import projected_langevin_sampling_amd as pkg

    return pkg._lib, pkg._lib.load()


A16 = 0x10000  # stand-ins for 16-byte aligned device pointers of calls that are refused before anything dereferences them
B16 = 0x20000
C16 = 0x30000


def route(L, lib, ldl, ldr, ldc, i, j, k=35, lptr=A16, rptr=B16):
    direct = ctypes.c_int32(-1)
    rc = lib.pls_gemm_tn_route(lptr, ldl, rptr, ldr, ldc, i, j, k, ctypes.byref(direct))
    return (L.GEMM_ROUTE_NAMES[rc] if rc >= 0 else rc), direct.value


def test_reported_limits_are_the_tables(lib):
    L, lib = lib
    # (29 columns: the last lane's pair reaches column 30, which costs the limit one double)
    for cols, want in ((128, 17895688), (144, 17895687), (16384, 17894604), (32768, 17893512), (1, 17895696), (29, 17895694),
                       (30, 17895694)):
        assert gemm_dma_max_ld(cols) == want
        assert lib.pls_ld_limit(L.LD_GEMM_TILES, 1, cols) == want
        pairs = cols + cols % 2
        assert (15 * want + pairs) * 8 <= 0x7FFFFFF0 < (15 * (want + 1) + pairs) * 8
    assert lib.pls_ld_limit(L.LD_GEMM_KSPLIT, 1, 1) == KSPLIT_MAX_LD - 1 == 2 ** 22 - 1
    assert lib.pls_ld_limit(L.LD_GEMM_DIRECT_STORE, 1, 1) == DIRECT_MAX_LD - 1 == 2 ** 21 - 1
    assert lib.pls_ld_limit(L.LD_SMALL_RANK, 1, 1) == SMALL_RANK_MAX_LD == 2 ** 23
    for m, cols, want in ((128, 96, 2113664), (257, 96, 2113664), (128, 80, 2113664), (128, 128, 2113663), (1024, 4096, 2113632),
                          (64, 96, 4260878), (2, 8, 268435416)):
        assert strip_max_ld(m, cols) == want
        assert lib.pls_ld_limit(L.LD_TRI_SOLVE, m, cols) == want
        rows = min(m, 128)
        assert ((rows - 1) * want + cols) * 8 <= 0x7FFFFF00 < ((rows - 1) * (want + 1) + cols) * 8
    assert lib.pls_ld_limit(L.LD_TRI_SOLVE, 1, 8) == 2 ** 63 - 1  # (a single row has no stride)
    for m, want in ((128, 2113663), (64, 4260879), (2, 268435452)):
        assert ipb_prep_max_ld(m) == want
        assert lib.pls_ld_limit(L.LD_IPB_PREP, m, 1) == want
        assert ((m - 1) * want + m) * 8 <= 0x7FFFFFF0 < ((m - 1) * (want + 1) + m) * 8
    assert lib.pls_ld_limit(99, 1, 1) == -1 and lib.pls_ld_limit(L.LD_GEMM_TILES, 0, 1) == -1
    # the k-split kernels reach (248 ld + 8 cols) bytes, the register -> global store (504 ld + 512): both routing limits
    # sit below what the offsets could take, so neither is ever the last safe value
    assert 248 * (KSPLIT_MAX_LD - 1) + 8 * 2 ** 24 < 0x7FFFFFF0 and 504 * (DIRECT_MAX_LD - 1) + 512 < 0x7FFFFFF0
    assert (31 * SMALL_RANK_MAX_LD + 128) * 8 <= 0x7FFFFF00 and (15 * SMALL_RANK_MAX_LD + 128) * 8 <= 0x7FFFFFF0


def test_gemm_route_on_either_side_of_every_limit(lib):
    L, lib = lib
    assert lib.pls_get_option(L.OPT_KSPLIT_MODE) == 1 and lib.pls_get_option(L.OPT_ROW_BLOCKS) == 1
    # 256 tiles of 128 x 128: the LDS-DMA k-loop takes ld = limit and refuses limit + 1 (odd: scalar loads) ... + 2
    i, j = 128, 32768
    li, lj = gemm_dma_max_ld(i), gemm_dma_max_ld(j)
    assert route(L, lib, li, j, j, i, j) == ("tiles_128", 1)
    assert route(L, lib, i, lj, j, i, j) == ("tiles_128", 1)
    assert route(L, lib, li + 2, j, j, i, j) == (-1, -1) and f"ldl={li + 2}".encode() in lib.pls_last_error()
    assert b"leading dimension" in lib.pls_last_error() and str(li).encode() in lib.pls_last_error()
    assert route(L, lib, i, lj + 2, j, i, j) == (-1, -1) and f"ldr={lj + 2}".encode() in lib.pls_last_error()
    # ... unless the operands take the scalar-load path (odd stride, or a base 8 bytes off): 64-bit pointers, no limit
    assert route(L, lib, li + 1, j, j, i, j) == ("tiles_128", 1)
    assert route(L, lib, li + 2 ** 16, j, j, i, j, lptr=A16 + 8) == ("tiles_128", 1)
    assert route(L, lib, i, lj + 2 ** 20, j, i, j, rptr=B16 + 8) == ("tiles_128", 1)
    # the register -> global store below 2^21, through LDS from there on
    assert route(L, lib, i, j, DIRECT_MAX_LD - 2, i, j) == ("tiles_128", 1)
    assert route(L, lib, i, j, DIRECT_MAX_LD, i, j) == ("tiles_128", 0)
    # few tiles: the k-split kernel below 2^22, the 64 x 64 tiles (64-bit pointers: no limit) from there on
    for ldl, ldr, want in ((128, 128, "ksplit_2"), (KSPLIT_MAX_LD - 2, 128, "ksplit_2"), (128, KSPLIT_MAX_LD - 2, "ksplit_2"),
                           (KSPLIT_MAX_LD, 128, "tiles_64"), (128, KSPLIT_MAX_LD, "tiles_64"), (li + 2 ** 16, 128, "tiles_64"),
                           (2 ** 40, 128, "tiles_64"), (129, 128, "tiles_64")):
        assert route(L, lib, ldl, ldr, 128, 128, 128) == (want, 1), (ldl, ldr)
    assert route(L, lib, 128, 128, DIRECT_MAX_LD, 128, 128) == ("ksplit_2", 0)
    # row blocks (I off the 128 grid, 256 tiles): the same DMA limit; an output stride of 2^21 hands the shape to the plain tiles
    i, j = 144, 16384
    li = gemm_dma_max_ld(i)
    assert li % 2 == 1
    assert route(L, lib, li - 1, j, j, i, j) == ("row_blocks", 1)
    assert route(L, lib, li + 1, j, j, i, j) == (-1, -1) and f"ldl={li + 1}".encode() in lib.pls_last_error()
    assert route(L, lib, i, j, DIRECT_MAX_LD - 2, i, j) == ("row_blocks", 1)
    assert route(L, lib, i, j, DIRECT_MAX_LD, i, j) == ("tiles_128", 0)
    assert route(L, lib, li, j, j, i, j) == ("tiles_128", 1)  # (odd: not the row blocks' operands, scalar loads)
    # forced k-split modes obey the same routing limit
    for mode, name in ((2, "ksplit_2"), (3, "ksplit_1"), (0, "tiles_64")):
        assert lib.pls_set_option(L.OPT_KSPLIT_MODE, mode) == 0
        try:
            assert route(L, lib, KSPLIT_MAX_LD - 2, 128, 128, 128, 128) == (name, 1)
            assert route(L, lib, KSPLIT_MAX_LD, 128, 128, 128, 128) == ("tiles_64", 1)
        finally:
            assert lib.pls_set_option(L.OPT_KSPLIT_MODE, 1) == 0
    assert lib.pls_gemm_tn_route(A16, 127, B16, 128, 128, 128, 128, 35, None) == -1  # (ldl < I)


def test_gemm_refuses_what_its_route_refuses(lib):
    L, lib = lib
    i, j = 128, 32768
    li, lj = gemm_dma_max_ld(i), gemm_dma_max_ld(j)
    assert lib.pls_ld_limit(L.LD_GEMM_TILES, 1, i) == li and lib.pls_ld_limit(L.LD_GEMM_TILES, 1, j) == lj
    for ldl, ldr, name in ((li + 2, j, f"ldl={li + 2}"), (i, lj + 2, f"ldr={lj + 2}"), (li + 2 ** 16, j, f"ldl={li + 2 ** 16}")):
        assert route(L, lib, ldl, ldr, j, i, j)[0] == -1  # (or the call below would launch)
        assert lib.pls_gemm_tn(A16, ldl, B16, ldr, C16, j, i, j, 35, 1.0, 0.0, None) == 1
        msg = lib.pls_last_error()
        assert b"leading dimension" in msg and name.encode() in msg, msg


def chol_desc(L, m, ldsf=None, ldsb=None):
    d = L.CholDesc()
    d.m = m
    d.Sf, d.ldsf = A16, m if ldsf is None else ldsf
    d.Sb, d.ldsb = B16, m if ldsb is None else ldsb
    return d


@pytest.mark.parametrize("m,j", [(128, 96), (257, 80), (1024, 4096), (64, 32)])
def test_substitution_entries_refuse_past_their_limit(lib, m, j):
    """pls_chol_solve, pls_chol_forward_solve and pls_chol_solve_ws where they substitute (no inverse factor in the descriptor),
    pls_chol_build_inverse: ldu / ldv / ldsf / ldsb one past strip_max_ld"""
    L, lib = lib
    lim, lim_s = strip_max_ld(m, j), strip_max_ld(m, m)
    assert lib.pls_ld_limit(L.LD_TRI_SOLVE, m, j) == lim and lib.pls_ld_limit(L.LD_TRI_SOLVE, m, m) == lim_s
    d = chol_desc(L, m)
    U, V = 0x40000, 0x50000

    def said(rc, *names):
        msg = lib.pls_last_error()
        assert rc == 1 and b"leading dimension" in msg and all(n.encode() in msg for n in names), (rc, msg)

    for ldu, ldv, name in ((lim + 1, j, f"ldu={lim + 1}"), (j, lim + 1, f"ldv={lim + 1}"), (lim + 2 ** 16, j, f"ldu={lim + 2 ** 16}")):
        said(lib.pls_chol_solve(d, U, ldu, j, V, ldv, None), name, str(lim))
        said(lib.pls_chol_forward_solve(d, U, ldu, j, V, ldv, None), name)
        said(lib.pls_chol_solve_ws(d, U, ldu, j, V, ldv, None, 0, None), name)
    said(lib.pls_chol_solve(chol_desc(L, m, ldsf=lim_s + 1), U, j, j, V, j, None), f"ldsf={lim_s + 1}", str(lim_s))
    said(lib.pls_chol_solve(chol_desc(L, m, ldsb=lim_s + 1), U, j, j, V, j, None), f"ldsb={lim_s + 1}")
    # the inverse factor is built by substitution on the identity: refused before the identity is written (even strides)
    over = (lim_s + 2) & ~1
    said(lib.pls_chol_build_inverse(d, U, over, V, m + (m & 1), None), f"ldlinv={over}", str(lim_s))
    said(lib.pls_chol_build_inverse(d, U, m + (m & 1), V, over, None), f"ldlinvt={over}")
    said(lib.pls_chol_build_inverse(chol_desc(L, m, ldsf=lim_s + 1), U, m + (m & 1), V, m + (m & 1), None), f"ldsf={lim_s + 1}")


@pytest.mark.parametrize("m,j", [(128, 96), (257, 80), (1024, 4096), (64, 32), (2, 8)])
def test_substitution_check_takes_the_limit_itself(lib, m, j):
    """pls_chol_solve_check is the check every substituting entry starts with (chol_solve_launch), without the launch behind
    it: ld = limit is accepted, limit + 1 refused by name -- for ldu, ldv, ldsf and ldsb, so `<` for `<=` in the guard fails"""
    L, lib = lib
    lim, lim_s = strip_max_ld(m, j), strip_max_ld(m, m)
    d = chol_desc(L, m)
    assert lib.pls_chol_solve_check(d, lim, j, lim) == 0, lib.pls_last_error()
    assert lib.pls_chol_solve_check(chol_desc(L, m, ldsf=lim_s, ldsb=lim_s), j, j, j) == 0, lib.pls_last_error()
    for ldu, ldv, dd, name in ((lim + 1, lim, d, f"ldu={lim + 1}"), (lim, lim + 1, d, f"ldv={lim + 1}"),
                               (j, j, chol_desc(L, m, ldsf=lim_s + 1, ldsb=lim_s), f"ldsf={lim_s + 1}"),
                               (j, j, chol_desc(L, m, ldsf=lim_s, ldsb=lim_s + 1), f"ldsb={lim_s + 1}")):
        assert lib.pls_chol_solve_check(dd, ldu, j, ldv) == 1
        msg = lib.pls_last_error()
        assert b"leading dimension" in msg and name.encode() in msg, msg


def test_small_rank_route_on_either_side_of_its_limit(lib):
    """pls_small_rank_route: small_rank_ok and sr_step_route_for, the predicates the ONB / IPB step and energy entries route
    by.  The fused kernels take the back-projection operand up to 2^23 and hand it to the contractions past it."""
    L, lib = lib
    assert lib.pls_get_option(L.OPT_SMALL_RANK_STEP) == 1 and lib.pls_get_option(L.OPT_SMALL_RANK_MAX) == 128
    SLABS, ONE = 1, 2
    kdim, n, j = 128, 256, 256  # (launch-bound: the one-launch step applies under option 1)
    for ld, want in ((kdim, SLABS | ONE), (SMALL_RANK_MAX_LD - 2, SLABS | ONE), (SMALL_RANK_MAX_LD, SLABS | ONE),
                     (SMALL_RANK_MAX_LD + 2, 0), (SMALL_RANK_MAX_LD + 2 ** 16, 0), (2 ** 40, 0),
                     (SMALL_RANK_MAX_LD - 1, 0)):  # (odd: rows off the 16-byte grid, not the limit)
        assert lib.pls_small_rank_route(A16, ld, kdim, n, B16, j) == want, ld
    assert lib.pls_small_rank_route(A16, SMALL_RANK_MAX_LD, kdim, n, B16 + 8, j) == SLABS  # (targets off the grid)
    assert lib.pls_small_rank_route(A16, SMALL_RANK_MAX_LD, kdim, 2 ** 20, B16, 4096) == SLABS  # (not launch-bound)
    assert lib.pls_small_rank_route(A16, SMALL_RANK_MAX_LD, 129, n, B16, j) == 0
    assert lib.pls_set_option(L.OPT_SMALL_RANK_STEP, 2) == 0
    try:
        assert lib.pls_small_rank_route(A16, SMALL_RANK_MAX_LD, kdim, 2 ** 20, B16, 4096) == SLABS | ONE
        assert lib.pls_small_rank_route(A16, SMALL_RANK_MAX_LD + 2, kdim, 2 ** 20, B16, 4096) == 0
    finally:
        assert lib.pls_set_option(L.OPT_SMALL_RANK_STEP, 1) == 0
    assert lib.pls_small_rank_route(A16, kdim - 1, kdim, n, B16, j) == -1  # (ldlb < kdim)


def ipb_desc(L, m, n, **ld):
    """a descriptor of stand-in pointers with the inverse factor, the substitution operators and LcT; ``ld``: field = value"""
    d = L.IpbDesc()
    d.m, d.n = m, n
    d.Kzx, d.ldkzx, d.Kxz, d.ldkxz = 0x100000, n, 0x200000, m
    d.LcT, d.Sf, d.Sb, d.Linv, d.LinvT = 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
    d.ldlct = d.ldsf = d.ldsb = d.ldlinv = d.ldlinvt = m
    for k, v in ld.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("m", [128, 64, 2])
def test_solve_and_noise_launch_route_on_either_side_of_its_limit(lib, m):
    """pls_ipb_prep_applies: the predicate of pls_ipb_step's two-launch route.  ldlinv / ldlinvt (and, for Philox noise, ldlct)
    up to ipb_prep_max_ld(m) keep the solve-and-noise launch; one past it the step takes the separate launches."""
    L, lib = lib
    assert lib.pls_get_option(L.OPT_IPB_PREP) == 1 and lib.pls_get_option(L.OPT_SOLVE_MODE) == 1
    lim = ipb_prep_max_ld(m)
    assert lib.pls_ld_limit(L.LD_IPB_PREP, m, 1) == lim
    for philox in (0, 1):
        assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256), philox) == 1
        assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256, ldlinv=lim, ldlinvt=lim, ldlct=lim), philox) == 1
        for field in ("ldlinv", "ldlinvt"):
            assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256, **{field: lim + 1}), philox) == 0, field
            assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256, **{field: lim + 2 ** 16}), philox) == 0, field
        assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256, ldlct=lim + 1), philox) == 1 - philox  # (LcT only colours drawn noise)
    assert lib.pls_set_option(L.OPT_IPB_PREP, 0) == 0
    try:
        assert lib.pls_ipb_prep_applies(ipb_desc(L, m, 256), 0) == 0
    finally:
        assert lib.pls_set_option(L.OPT_IPB_PREP, 1) == 0


def test_whitened_generic_step_refuses_ldawa_past_its_limit(lib):
    """pls_ipb_whitened_generic_applies and the entry's own refusal.  A call that is not refused would launch, so the entry is
    called with targets 8 bytes off the 16-byte grid, which it refuses AFTER the stride check: at ldawa = 2^23 the message is
    that refusal and does not speak of a leading dimension, one even value further it names ldawa."""
    L, lib = lib
    m, n, j = 64, 16, 256
    cost = L.CostDesc()
    cost.cost, cost.link, cost.deriv_mode = L.COST_GAUSSIAN, L.LINK_IDENTITY, L.DERIV_REFERENCE
    cost.p[0] = 0.25
    S, OUT, WS, Y = 0x800000, 0x900000, 0xA00000, 0xB00000

    def step(d, y):
        return lib.pls_ipb_whitened_generic_step(d, cost, y, S, j, j, 2.0 ** -21, None, None, OUT, j, L.OUT_DELTA, None, WS, 1 << 30, None)

    at, over = ipb_desc(L, m, n, Awa=0xC00000, ldawa=SMALL_RANK_MAX_LD), ipb_desc(L, m, n, Awa=0xC00000, ldawa=SMALL_RANK_MAX_LD + 2)
    assert lib.pls_ipb_whitened_generic_applies(ipb_desc(L, m, n, Awa=0xC00000, ldawa=m), Y, j) == 1
    assert lib.pls_ipb_whitened_generic_applies(at, Y, j) == 1
    assert lib.pls_ipb_whitened_generic_applies(over, Y, j) == 0
    assert lib.pls_ipb_whitened_generic_applies(ipb_desc(L, m, n, Awa=0xC00000, ldawa=SMALL_RANK_MAX_LD + 2 ** 16), Y, j) == 0
    assert lib.pls_ipb_whitened_generic_applies(at, Y + 8, j) == 0  # (what lets the entry be called below)
    assert step(at, Y + 8) == 1
    msg = lib.pls_last_error()
    assert b"leading dimension" not in msg and b"ldawa" not in msg and b"16-byte aligned targets" in msg, msg
    for d, y in ((over, Y + 8), (over, Y)):
        assert step(d, y) == 1
        msg = lib.pls_last_error()
        assert b"leading dimension" in msg and f"ldawa={SMALL_RANK_MAX_LD + 2}".encode() in msg and str(SMALL_RANK_MAX_LD).encode() in msg, msg
