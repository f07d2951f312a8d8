"""GPU: every entry that is LENT memory stays inside it and reads only what it wrote in the same call.

The workspaces sized by the pls_*_workspace_bytes queries, the side buffers whose size include/plship.h states (energy_in,
energy_sums, energy_sums16, energy_prev, the lagged partial rows, step_sync, energy_sync, the Winograd planes) and the outputs
are each one workspace_guards.Guarded: exactly the queried bytes between two guards of at least 4 MiB that hold a fixed
pattern.  For every cell three properties:

  containment   with exactly the queried bytes the call returns PLS_OK, runs the route the cell names (Timeline tags), leaves
                every guard intact, writes every output entry the header says it writes and leaves caller-owned counters zero;
  independence  the outputs are bit-identical with the lent regions filled with NaN, 1e300 and 0.0, and equal to the exact
                fixtures' expected values (step_fixtures) under the fixtures' own assertion;
  size honesty  one double less than the smallest size the entry documents gives PLS_ERR_WORKSPACE_TOO_SMALL with every guard
                intact -- or, where a smaller workspace means another route (one launch -> general, Winograd -> plain, products
                -> substitution), that route by its tags, with the same properties.

Nothing here has a tolerance of its own: bit equality, or the exact fixtures' assertion (assert_exact: the step bit for bit,
the energy by-product at 1e-13 or bit for bit where the fixture proves it exact)."""
import copy
import ctypes
import math

import pytest
import torch

import base_kernel_calls as bkc
import numpy as np
import svgp_quadrature_truth
import svgp_truth
from step_fixtures import EXACT_ETA, ExactProblem, assert_exact, exact_ipb, option, probe_winograd, wino_one_chunk_bytes
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks
from workspace_guards import FILLS, SENTINEL, SENTINEL_BITS, Guarded, GuardedMatrix, same_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
OK, TOO_SMALL = 0, 3


def cdiv(a, b):
    return -(-a // b)


def padded(t):
    """device copy of the host matrix ``t`` inside NaN padding columns: an even leading dimension > its width (rows stay
    16-byte aligned, so the tilings of the contiguous case are the ones that run)"""
    rows, cols = t.shape
    wide = torch.full((rows, cols + 2 + cols % 2), NAN, dtype=F64, device="cuda")
    wide[:, :cols] = t.cuda()
    return wide[:, :cols]


def test_the_guards_report_a_double_written_by_torch_on_either_side():
    """the helper does not pass vacuously on the device: one double just behind and just in front of the region"""
    g = Guarded(1000 * 8, NAN)
    g.assert_intact("untouched")
    assert g.ptr % 256 == 0 and g.guard == 4 << 20 and g.f64().isnan().all()
    words = g._words.view(F64)
    words[g.end // 8] = 1.0
    assert g.first_damage() == g.nbytes
    with pytest.raises(AssertionError, match="0 bytes behind"):
        g.assert_intact("behind")
    words[g.end // 8] = SENTINEL
    g.assert_intact("repaired")
    words[g.start // 8 - 1] = 1.0
    assert g.first_damage() == -8
    odd = Guarded(7 * 4, 0.0)  # 28 bytes: the region ends inside a word
    odd.assert_zero("counters")
    odd.view(torch.int32)[6] = 5
    odd.assert_intact("a store to the last counter")
    with pytest.raises(AssertionError, match="byte 24"):
        odd.assert_zero("counters")
    odd._bytes[odd.end] = 1
    assert odd.first_damage() == 28
    out = GuardedMatrix(3, 5, 8)
    with pytest.raises(AssertionError, match="never written"):
        out.assert_written("nothing stored")
    out.matrix().fill_(2.0)
    out.assert_written("stored")
    out.assert_intact("stored")
    out.f64()[5] = 0.0  # (row 0, padding column 0)
    with pytest.raises(AssertionError, match="padding"):
        out.assert_written("a store into the padding")


# -------------------------------------------------------------------------------------------------------------------------
# one step call with everything it is lent inside guards
class Res:
    pass


def step_call(P, gb, cost, u, noise, fill, force_generic=False, whitened=False, energy=True, sums=False, sums16=False,
              esync=False, step_sync=None, ws_bytes=None, eta=EXACT_ETA, lag=None, new_state=False, wg=None):
    """One call of the basis' step entry (StepRoute.call: the C ABI) on the particles ``u``.  ``ws_bytes``: the workspace
    (default: what the route asks); ``step_sync``: "caller" = guarded counters in the block descriptor, None = the library
    carves them from the workspace; ``lag``: dict(out=Guarded | None, prev=Guarded | None, flush=bool) for the lagged energies;
    ``wg``: (Guarded planes) through the _wg entries."""
    L = P.pkg._lib
    lib = L.load()
    mk, j = u.shape
    r = gb._route(cost, j, force_generic, whitened)
    if ws_bytes is None:
        ws_bytes = r.workspace_bytes(energy and lag is None)
    res = Res()
    g = res.guards = {}
    res.zeroed, res.outputs = [], []
    res.ws_bytes = ws_bytes
    ws = g["workspace"] = Guarded(ws_bytes, fill) if ws_bytes else None
    flush = bool(lag and lag.get("flush"))
    ldo = j + 2 + j % 2
    out = res.out = None
    if not flush:
        out = res.out = g["out"] = GuardedMatrix(mk, j, ldo)
    e = None
    if energy and lag is None:
        e = g["energy_in"] = Guarded(8 * j, SENTINEL)
        res.outputs.append("energy_in")
    bd, eta_word = None, torch.full((1,), float(eta), dtype=F64, device="cuda")
    if sums or sums16 or esync or step_sync == "caller" or lag is not None or r.fn is None:
        bd = L.BlockDesc()
        bd.block_cols, bd.eta = j, eta_word.data_ptr()
        if sums:
            g["energy_sums"] = Guarded(8 * cdiv(j, 256), SENTINEL)
            bd.energy_sums = g["energy_sums"].ptr
            res.outputs.append("energy_sums")
        if sums16:
            g["energy_sums16"] = Guarded(8 * cdiv(j, 16), SENTINEL)
            bd.energy_sums16 = g["energy_sums16"].ptr
            res.outputs.append("energy_sums16")
        if esync:
            g["energy_sync"] = Guarded(4 * cdiv(j, 256), 0.0)
            bd.energy_sync = g["energy_sync"].ptr
            res.zeroed.append("energy_sync")
        if step_sync == "caller":
            g["step_sync"] = Guarded(4 * int(lib.pls_step_sync_words(j)), 0.0)
            bd.step_sync = g["step_sync"].ptr
            res.zeroed.append("step_sync")
        if lag is not None:
            if lag.get("out") is not None:
                g["energy_partials"] = lag["out"]
                bd.energy_partials = lag["out"].ptr
            if lag.get("prev") is not None:
                g["energy_partials_prev"] = lag["prev"]
                bd.energy_partials_prev = lag["prev"].ptr
                g["energy_prev"] = Guarded(8 * j, SENTINEL)
                g["energy_sums_prev"] = Guarded(8 * cdiv(j, 256), SENTINEL)
                bd.energy_prev, bd.energy_sums_prev = g["energy_prev"].ptr, g["energy_sums_prev"].ptr
                res.outputs += ["energy_prev", "energy_sums_prev"]
            bd.energy_flush = 1 if flush else 0
    nd = noise.desc()
    mode = L.OUT_NEW_STATE if new_state else L.OUT_DELTA
    fn = r.fn if bd is None else r.fn_blocks
    mid = (float(eta),) if bd is None else (*r.blocks_head, bd)
    tail = r.tail
    if wg is not None:  # the _wg entries with the caller's planes in the place of the basis' own
        fn = getattr(lib, "pls_onb_step_wg" if bd is None else "pls_onb_step_blocks_wg")
        tail = (r.tail[0], wg.ptr, wg.nbytes)
    with L.Timeline(512) as tl:
        res.rc = fn(*r.head, u.data_ptr(), L.ld(u), j, *mid, nd, None if out is None else out.ptr, 0 if out is None else ldo, mode,
                    *tail, None if e is None else e.ptr, None if ws is None else ws.ptr, ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    res.error = lib.pls_last_error().decode() if res.rc else ""
    res.tags = [name for name, _ in tl.records]
    res.entry = r.entry if bd is None else r.blocks_entry
    res.keep = (eta_word, nd, noise, u, r)
    return res


def intact(res, what):
    for name, gd in res.guards.items():
        if gd is not None:
            gd.assert_intact(f"{what}: {name}")


def contained(res, what):
    """PLS_OK, every guard intact, every output written, caller-owned counters zero again"""
    assert res.rc == OK, f"{what}: {res.entry} returned {res.rc}: {res.error}"
    intact(res, what)
    if res.out is not None:
        res.out.assert_written(f"{what}: out")
    for name in res.outputs:
        res.guards[name].assert_written(f"{what}: {name}")
    for name in res.zeroed:
        res.guards[name].assert_zero(f"{what}: {name}")


def refused(res, what):
    """PLS_ERR_WORKSPACE_TOO_SMALL and nothing touched"""
    assert res.rc == TOO_SMALL, f"{what}: {res.entry} returned {res.rc} ({res.error}) for a workspace of {res.ws_bytes} bytes"
    intact(res, what)
    for name in res.zeroed:
        res.guards[name].assert_zero(f"{what}: {name}")


def bits_of(res):
    d = {} if res.out is None else {"out": res.out.matrix(torch.int64).clone()}
    for name in res.outputs:
        d[name] = res.guards[name].bits().clone()
    return d


def assert_same(first, res, what):
    a, b = bits_of(first), bits_of(res)
    assert a.keys() == b.keys()
    for name in a:
        diff = (a[name] != b[name]).nonzero()
        assert diff.numel() == 0, f"{what}: {name} depends on what the lent memory held: {diff.shape[0]} entries differ, first {diff[0].tolist()}"


def count(tags, name):
    return sum(1 for t in tags if t == name)


def cell(P, ex, gb, cost, u, noise, what, route=None, check=None, cols=None, **kw):
    """containment and independence of one configuration: the call under the three fills; ``route(tags)`` asserts the route,
    ``check(out, energy)`` the fixture's expectation (default: assert_exact)"""
    first = None
    for fill in FILLS:
        res = step_call(P, gb, cost, u, noise, fill, **kw)
        tag = f"{what} [fill {fill}, workspace {res.ws_bytes} bytes, launches {res.tags}]"
        contained(res, tag)
        if route is not None:
            route(res.tags)
        if first is None:
            first = res
            print(f"{what}: {res.entry}, workspace {res.ws_bytes} bytes, launches {sorted(set(res.tags))}")
            e = res.guards["energy_in"].f64() if "energy_in" in res.guards else None
            if check is not None:
                check(res.out.matrix(), e)
            elif res.out is not None:
                assert_exact(ex, res.out.matrix(), cols, energy=e, eta=kw.get("eta", EXACT_ETA), new_state=kw.get("new_state", False),
                             what=what)
        else:
            assert_same(first, res, tag)
    return first


def sums_follow(P, res, what):
    """energy_sums / energy_sums16 are the library's fixed-order sums of energy_in (pls_chunk_sums, pls_sums16), bit for bit"""
    L = P.pkg._lib
    lib = L.load()
    e = res.guards["energy_in"].f64().clone()
    j = e.numel()
    if "energy_sums" in res.guards:
        want = torch.empty(cdiv(j, 256), dtype=F64, device="cuda")
        L.check(lib.pls_chunk_sums(e.data_ptr(), j, want.data_ptr(), L.stream_ptr()), "pls_chunk_sums")
        assert same_bits(res.guards["energy_sums"].f64(), want), f"{what}: energy_sums"
    if "energy_sums16" in res.guards:
        want = torch.empty(cdiv(j, 16), dtype=F64, device="cuda")
        L.check(lib.pls_sums16(e.data_ptr(), j, want.data_ptr(), L.stream_ptr()), "pls_sums16")
        assert same_bits(res.guards["energy_sums16"].f64(), want), f"{what}: energy_sums16"


def is_fast(tags):
    assert "gemm_langevin_gaussian" in tags and "gemm_cost_deriv" not in tags and "small_rank_step" not in tags, tags


def is_one_launch(tags):
    assert tags == ["small_rank_step"], tags


def is_slab_kernels(tags):
    assert "small_rank_drift" in tags and "small_rank_step" not in tags and "gemm_cost_deriv" not in tags, tags


def is_general(chunks):
    def route(tags):
        assert count(tags, "gemm_cost_deriv") == chunks, (chunks, tags)
        assert not any(t.startswith("small_rank") or t == "gemm_langevin_gaussian" for t in tags), tags

    return route


# -------------------------------------------------------------------------------------------------------------------------
# the launch plans of the library, written out again: which launch a cell must have taken is asserted from the same arithmetic
def plan_split_k(i, j, k):
    """csrc/step_plan.h plan_split_k: split-K slabs of the back-projection D (i x j) over k rows"""
    tiles = cdiv(i, 128) * cdiv(j, 128)
    s = min(max(cdiv(512, tiles) if tiles < 512 else 1, cdiv(k, 16384)), 16)
    if s > 1:
        def waste(sl):
            return math.ceil(tiles * sl / 512.0) / (tiles * sl / 512.0)

        best = s
        for sl in range(s + 1, min(16, s + 4) + 1):
            if waste(sl) < waste(best) - 0.03:
                best = sl
        s = best
    while s > 1 and k // s < (256 if tiles < 64 else 1024):
        s -= 1
    return cdiv(k, cdiv(cdiv(k, s), 16) * 16)


def back_projection(mk, j, rows, row_blocks_on):
    """(launch, slabs) of stream_drift's back-projection for chunks of ``rows`` rows (csrc/plship.hip stream_drift, gemm_rows_ok;
    operands 16-byte aligned with even leading dimensions, as the tests here build them): "rows" = one launch of
    gemm_tn_f64_rows.h, "pieces" = 128-row tiles plus 64- / 32- / 16-row remainder launches, "plain" = one launch of plain tiles"""
    slabs = plan_split_k(mk, j, rows)
    big = cdiv(mk, 128) * cdiv(j, 128) * slabs >= 256
    tiles, blocks = cdiv(mk, 128), cdiv(mk, 16)
    if row_blocks_on and mk > 128 and mk % 128 and j % 2 == 0 and j >= 128 and big and (tiles == 2 or tiles * cdiv(blocks, tiles) - blocks <= 1):
        return "rows", slabs
    if mk >= 128 and 0 < mk % 128 <= 112 and big:
        return "pieces", slabs
    return "plain", slabs


def piece_launches(mk):
    """launches of the "pieces" back-projection per chunk: the 128-row tiles, then pieces of at most 64 rows"""
    launches, left = 1, mk % 128
    while left > 0:
        left -= min(left, 64) if left > 32 else left
        launches += 1
    return launches


def one_launch_slabs(j, n, k):
    """csrc/small_rank_step.h small_rank_step_splits: row slabs per column block of the one-launch step"""
    ncb, kb, rounds = cdiv(j, 16), cdiv(k, 16), cdiv(n, 64)
    s = 1
    if rounds * max(0.28 * kb, 1.1) > 6.0:
        s = max(1, min(256 // ncb, rounds // 2, 64))
    rows = max(cdiv(cdiv(n, s), 64) * 64, 64)
    if s > 1:
        down = max((n // s) // 64 * 64, 128)
        if down < rows and cdiv(n, down) <= (16 if kb <= 2 else 12 if kb <= 4 else 8) and ncb * cdiv(n, down) <= 256:
            rows = down
    return max(cdiv(n, rows), 1)


_onb = {}


def onb(P, mk, n, j):
    key = (mk, n, j)
    if key not in _onb:
        if len(_onb) >= 3:
            _onb.clear()
        ex = ExactProblem(mk, n, j, seed=mk + n + j)
        _onb[key] = (ex, ex.basis(P), ex.cost(P), padded(ex.u), P.basis.NoiseSpec(injected=padded(ex.xi)))
    return _onb[key]


# -------------------------------------------------------------------------------------------------------------------------
# pls_onb_step / _blocks: the Gaussian fast path
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("mk,n,j", [(100, 300, 333), (129, 300, 1100)])
def test_onb_fast_path(P, mk, n, j, mode):
    """energy_in direct (finishing launch), energy_sums + energy_sync (the step launch finishes), lagged over two alternating
    partial buffers, then energy_flush -- under every k-split mode"""
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, xi = onb(P, mk, n, j)
    pbytes = int(lib.pls_energy_partials_bytes(mk, j))
    with ksplit(P, mode):
        what = f"fast path {mk}x{n}x{j}, k-split {mode}"
        plain = cell(P, ex, gb, cost, u, xi, f"{what}: no energies", route=is_fast, energy=False)
        assert plain.ws_bytes == 0
        direct = cell(P, ex, gb, cost, u, xi, f"{what}: direct", route=is_fast, sums=True, sums16=True)
        assert direct.ws_bytes == pbytes == 2 * cdiv(mk, 128) * j * 8
        sums_follow(P, direct, what)
        assert same_bits(direct.out.matrix(), plain.out.matrix()), "asking for the energies moved the step"
        fused = cell(P, ex, gb, cost, u, xi, f"{what}: sums + sync", route=is_fast, sums=True, esync=True)
        assert fused.tags == ["gemm_langevin_gaussian"], f"the step launch did not finish the energies itself: {fused.tags}"
        assert_same(cell(P, ex, gb, cost, u, xi, f"{what}: direct again", route=is_fast, sums=True), fused, f"{what}: sums + sync")
        # lagged: launch A leaves its partial rows, launch B finishes them at its start and leaves its own, the flush finishes those
        for fill in FILLS:
            bufs = [Guarded(pbytes, fill), Guarded(pbytes, fill)]
            a = step_call(P, gb, cost, u, xi, fill, lag=dict(out=bufs[0]))
            contained(a, f"{what}: lagged, first launch")
            assert a.ws_bytes == 0 and same_bits(a.out.matrix(), plain.out.matrix())
            b = step_call(P, gb, cost, u, xi, fill, lag=dict(out=bufs[1], prev=bufs[0]))
            contained(b, f"{what}: lagged, second launch")
            assert same_bits(b.out.matrix(), plain.out.matrix())
            f = step_call(P, gb, cost, u, xi, fill, lag=dict(prev=bufs[1], flush=True))
            contained(f, f"{what}: flush")
            for r in (b, f):
                assert same_bits(r.guards["energy_prev"].f64(), direct.guards["energy_in"].f64()), f"{what}: lagged energies, fill {fill}"
                assert same_bits(r.guards["energy_sums_prev"].f64(), direct.guards["energy_sums"].f64()), f"{what}: lagged sums"
        # size honesty: the header's 2 cdiv(mk, 128) j doubles hold every tiling; a launch of 64-row tiles leaves cdiv(mk, 64) rows
        # (csrc/step_plan.h gaussian_partial_rows) and may take a workspace of that many: never fewer
        small = step_call(P, gb, cost, u, xi, NAN, ws_bytes=pbytes - 8)
        if small.rc == OK:
            assert cdiv(mk, 64) < 2 * cdiv(mk, 128), f"{what}: one double short of the documented size was accepted"
            contained(small, f"{what}: one double short of the documented size")
            assert_same(direct_only(direct), direct_only(small), f"{what}: short workspace")
            small = step_call(P, gb, cost, u, xi, NAN, ws_bytes=cdiv(mk, 64) * j * 8 - 8)
        refused(small, f"{what}: one double short")


def shrinking(P, ex, gb, cost, u, xi, q128, full, what, routes, **kw):
    """Workspaces below the 128-row query of a basis with at most 128 functions, whose query is the larger of two routes'
    layouts: q128 - 8 bytes, then 3/4, 1/2, 1/4, 1/8 of it, then one double.  At every size the call either runs one of
    ``routes`` (its launches in order) contained and with the bits of ``full``, or is refused and touches nothing; once a size
    is refused every smaller one is; one double is refused."""
    was_refused = False
    for ws_bytes in [q128 - 8] + [q128 * k // 64 * 8 for k in (6, 4, 2, 1)] + [8]:
        res = step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=ws_bytes, **kw)
        print(f"{what}: workspace {ws_bytes} of {q128} bytes -> status {res.rc}, launches {res.tags}")
        if res.rc == OK:
            assert not was_refused, f"{what}: {ws_bytes} bytes accepted after a larger workspace was refused"
            assert res.tags in [list(r) for r in routes], res.tags
            contained(res, f"{what}, workspace {ws_bytes}")
            assert_same(direct_only(full), direct_only(res), f"{what}, workspace {ws_bytes}")
        else:
            refused(res, f"{what}, workspace {ws_bytes}")
            was_refused = True
    assert was_refused, f"{what}: a workspace of one double was accepted"


def direct_only(res):
    """a view of a result that compares out and energy_in alone"""
    r = Res()
    r.out, r.guards, r.outputs = res.out, res.guards, ["energy_in"]
    return r


# -------------------------------------------------------------------------------------------------------------------------
# the one-launch step and the slab kernels of small_rank.h
@pytest.mark.parametrize("n,mk,j", [(40, 12, 5), (333, 17, 37), (900, 128, 48), (2600, 64, 530)])
def test_onb_one_launch_step(P, n, mk, j):
    """csrc/small_rank_step.h with the caller's step_sync and with counters carved from the workspace (a memset node in front),
    each with energy_sums16 and with energy_sums; every shape but (40, 12, 5) takes several row slabs per column block, (2600, 64,
    530) seven (asserted from the plan, one_launch_slabs, and from the bytes the launch accepts)"""
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, xi = onb(P, mk, n, j)
    query = int(lib.pls_onb_step_workspace_bytes(gb._desc(), j, n))
    ns = one_launch_slabs(j, n, mk)
    assert (ns > 1) == ((n, mk, j) != (40, 12, 5)) and (ns >= 7 if n == 2600 else True), f"{ns} row slabs planned for {n}x{mk}x{j}"
    slab_bytes = cdiv(cdiv(j, 16) * ns * (mk + 1) * 16 * 8, 256) * 256 if ns > 1 else 0
    with option(P, L.OPT_SMALL_RANK_STEP, 2):
        # the slabs are the whole layout when the caller brings the counters: exactly their bytes run the one launch, one double
        # less does not (the general route takes over where its own layout fits, else the call is refused)
        exact = step_call(P, gb, cost, u, xi, NAN, force_generic=True, energy=False, step_sync="caller", ws_bytes=slab_bytes)
        contained(exact, f"one launch {n}x{mk}x{j} in the {slab_bytes} bytes of its {ns} slabs")
        is_one_launch(exact.tags)
        assert_exact(ex, exact.out.matrix(), what=f"one launch {n}x{mk}x{j} in the bytes of its slabs")
        if slab_bytes:
            short = step_call(P, gb, cost, u, xi, NAN, force_generic=True, energy=False, step_sync="caller", ws_bytes=slab_bytes - 8)
            assert "small_rank_step" not in short.tags, f"the one-launch step ran {ns} slabs in {slab_bytes - 8} bytes"
            if short.rc == OK:
                contained(short, "one double short of the slabs: the general route")
                assert same_bits(short.out.matrix(), exact.out.matrix())
            else:
                refused(short, "one double short of the slabs")
        first = None
        for sync in ("caller", None):
            for kw in (dict(sums16=True), dict(sums=True), dict(energy=False)):
                what = f"one launch {n}x{mk}x{j}, step_sync {sync}, {kw}"
                res = cell(P, ex, gb, cost, u, xi, what, route=is_one_launch, force_generic=True, step_sync=sync, **kw)
                assert res.ws_bytes == query
                if kw.get("energy", True):
                    sums_follow(P, res, what)
                first = first or res
                assert same_bits(res.out.matrix(), first.out.matrix()), f"{what}: the step moved"
        # M_k <= 128: the 128-row query is the larger of the general route's layout and the one-launch layout, so one double less
        # may still hold one of them -- then that route runs, by its tags -- and a workspace too small for both is refused
        q128 = int(lib.pls_onb_step_workspace_bytes(gb._desc(), j, 128))
        shrinking(P, ex, gb, cost, u, xi, q128, first, f"one launch {n}x{mk}x{j}", (["small_rank_step"], ["small_rank_drift", "langevin_update"]),
                  step_sync=None, sums=True)  # (counters carved from the workspace for the chunk sums: the layout is never empty)
    # the other route: option 0 = the slab kernels + update launch in the same workspace
    with option(P, L.OPT_SMALL_RANK_STEP, 0):
        cell(P, ex, gb, cost, u, xi, f"slab kernels at {n}x{mk}x{j}", route=is_slab_kernels, force_generic=True, sums=True, sums16=True)


@pytest.mark.parametrize("n,mk,j", [(3000, 30, 40), (1530, 120, 200)])
def test_onb_slab_kernels(P, n, mk, j):
    """PLS_OPT_SMALL_RANK_STEP 0: small_rank.h's row slabs, the column reduce of the energies, the update launch"""
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, xi = onb(P, mk, n, j)
    q128, qn = (int(lib.pls_onb_step_workspace_bytes(gb._desc(), j, c)) for c in (128, n))
    with option(P, L.OPT_SMALL_RANK_STEP, 0):
        for kw in (dict(), dict(energy=False), dict(sums=True, sums16=True)):
            what = f"slab kernels {n}x{mk}x{j} {kw}"
            res = cell(P, ex, gb, cost, u, xi, what, route=is_slab_kernels, force_generic=True, **kw)
            assert res.ws_bytes == qn
            if kw.get("sums"):
                sums_follow(P, res, what)
        whole = cell(P, ex, gb, cost, u, xi, "slab kernels, 128-row query", route=is_slab_kernels, force_generic=True, ws_bytes=q128)
        again = cell(P, ex, gb, cost, u, xi, "slab kernels again", route=is_slab_kernels, force_generic=True)
        assert_same(direct_only(whole), direct_only(again), "slab kernels: the 128-row workspace")
        shrinking(P, ex, gb, cost, u, xi, q128, whole, f"slab kernels {n}x{mk}x{j}", (["small_rank_drift", "langevin_update"],))


# -------------------------------------------------------------------------------------------------------------------------
# the general GEMM route
def general_cells(P, ex, gb, cost, u, xi, what, n, chunk_rows=512):
    """whole and in chunks of ``chunk_rows`` rows (a short last chunk), with and without energy_in, with the appended sums; the
    128-row query, a size between it and the all-rows query, and one double short of it"""
    L = P.pkg._lib
    lib = L.load()
    j = u.shape[1]
    desc = gb._route(cost, j, True).head[0]
    q128, qc, qn = (int(lib.pls_onb_step_workspace_bytes(desc, j, c)) for c in (128, chunk_rows, n))
    assert q128 < qc < qn
    whole = cell(P, ex, gb, cost, u, xi, f"{what}: whole", route=is_general(1), force_generic=True, sums=True, sums16=True)
    assert whole.ws_bytes == qn
    sums_follow(P, whole, what)
    bare = cell(P, ex, gb, cost, u, xi, f"{what}: whole, no energies", route=is_general(1), force_generic=True, energy=False)
    assert same_bits(bare.out.matrix(), whole.out.matrix()), f"{what}: asking for the energies moved the step"
    chunks = cdiv(n, chunk_rows)
    assert n % chunk_rows, "the last chunk must be short"
    part = cell(P, ex, gb, cost, u, xi, f"{what}: chunks of {chunk_rows}", route=is_general(chunks), force_generic=True, sums=True,
                sums16=True, ws_bytes=qc)
    sums_follow(P, part, what)
    cell(P, ex, gb, cost, u, xi, f"{what}: chunks of {chunk_rows}, no energies", route=is_general(chunks), force_generic=True,
         energy=False, ws_bytes=qc)
    # between two chunk sizes: the largest multiple of 128 that fits
    between = cell(P, ex, gb, cost, u, xi, f"{what}: between the queries", route=is_general(chunks), force_generic=True,
                   ws_bytes=qc + (int(lib.pls_onb_step_workspace_bytes(desc, j, chunk_rows + 128)) - qc) // 16 * 8)
    least = cell(P, ex, gb, cost, u, xi, f"{what}: chunks of 128", route=is_general(cdiv(n, 128)), force_generic=True, ws_bytes=q128)
    # (the exact problem is exact in any summation order: chunked and whole agree bit for bit in the step)
    for r in (part, between, least):
        assert same_bits(r.out.matrix(), whole.out.matrix()), f"{what}: the chunked step differs from the whole one"
    refused(step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=q128 - 8), f"{what}: one double short of the 128-row query")


def test_onb_general_route(P):
    ex, gb, cost, u, xi = onb(P, 200, 1500, 333)
    general_cells(P, ex, gb, cost, u, xi, "general 200x1500x333", 1500)


@pytest.mark.parametrize("mode", [2, 3])
def test_onb_general_route_under_the_k_split_kernels(P, mode):
    ex, gb, cost, u, xi = onb(P, 200, 1500, 333)
    with ksplit(P, mode):
        general_cells(P, ex, gb, cost, u, xi, f"general 200x1500x333, k-split {mode}", 1500)


@pytest.mark.parametrize("mk", [129, 200, 300])
def test_onb_general_route_row_blocks(P, mk):
    """The issue's shapes under PLS_OPT_ROW_BLOCKS 1 (J = 333) and 0 (J = 1100).  At N = 1500 the back-projection stays below 256
    tiles with its split-K slabs, so stream_drift takes one launch of plain tiles under either option -- asserted from the plan;
    the row-block launch and the remainder pieces themselves: test_onb_row_block_and_remainder_launches."""
    for j, mode in ((333, True), (1100, False)):
        for rows in (1500, 512, 128):
            assert back_projection(mk, j, rows, mode)[0] == "plain"
    with row_blocks(P, 1):
        ex, gb, cost, u, xi = onb(P, mk, 1500, 333)
        general_cells(P, ex, gb, cost, u, xi, f"general {mk}x1500x333, row blocks on", 1500)
    with row_blocks(P, 0):
        ex, gb, cost, u, xi = onb(P, mk, 1500, 1100)
        general_cells(P, ex, gb, cost, u, xi, f"general {mk}x1500x1100, row blocks off", 1500)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("mk", [129, 200, 300])
def test_onb_row_block_and_remainder_launches(P, mk, mode):
    """N = 8500, J = 1100: 16 split-K slabs put the back-projection above 256 tiles, where stream_drift takes the row-block launch
    (PLS_OPT_ROW_BLOCKS 1; M_k = 129, 200: two equal-height tile rows) or the 128-row tiles plus remainder pieces (option 0, and
    M_k = 300 under either option: three tile rows of 7 blocks would pad 2 blocks, so gemm_rows_ok declines).  Whole, and in
    chunks of 4224 rows (two full chunks, then 52 rows that reach only the first slab).  The launch is asserted from the plan's
    arithmetic (back_projection) and, for the pieces, from the number of storing launches per chunk."""
    L = P.pkg._lib
    lib = L.load()
    n, j, chunk = 8500, 1100, 4224
    ex, gb, cost, u, xi = onb(P, mk, n, j)
    desc = gb._route(cost, j, True).head[0]
    q128, qc, qn = (int(lib.pls_onb_step_workspace_bytes(desc, j, c)) for c in (128, chunk, n))
    want = "rows" if mode and mk < 300 else "pieces"
    results = []
    with row_blocks(P, mode):
        for rows, ws_bytes in ((n, qn), (chunk, qc)):
            launch, slabs = back_projection(mk, j, rows, bool(mode))
            assert (launch, slabs) == (want, 16) and slabs <= plan_split_k(mk, j, n), (launch, slabs)
            chunks = cdiv(n, rows)
            stores = chunks * (piece_launches(mk) if launch == "pieces" else 1)
            assert launch != "pieces" or stores >= 2 * chunks

            def route(tags):
                assert count(tags, "gemm_cost_deriv") == chunks and count(tags, "gemm_store") == stores, (chunks, stores, tags)

            what = f"general {mk}x{n}x{j}, row blocks {mode}, chunks of {rows}: {launch}"
            res = cell(P, ex, gb, cost, u, xi, what, route=route, force_generic=True, sums=True, sums16=True, ws_bytes=ws_bytes)
            sums_follow(P, res, what)
            bare = cell(P, ex, gb, cost, u, xi, f"{what}, no energies", route=route, force_generic=True, energy=False, ws_bytes=ws_bytes)
            assert same_bits(bare.out.matrix(), res.out.matrix())
            results.append(res)
        assert_same(direct_only(results[0]), direct_only(results[1]), f"general {mk}x{n}x{j}: chunked against whole")
        refused(step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=q128 - 8), f"general {mk}x{n}x{j}: one double short")


def test_onb_winograd_route(P):
    """the route's smallest admissible shape, the planes of pls_onb_winograd_prepare in a guarded buffer of
    pls_onb_winograd_bytes; a workspace too small for its chunks of 8192 paired rows: the plain route"""
    L = P.pkg._lib
    lib = L.load()
    mk, n, j = 512, 16384, 2048
    ex = ExactProblem(mk, n, j, seed=5)
    gb, cost = ex.basis(P), ex.cost(P)
    u, xi = padded(ex.u), P.basis.NoiseSpec(injected=padded(ex.xi))
    desc = gb._desc()
    pbytes = int(lib.pls_onb_winograd_bytes(desc))
    assert pbytes == 4 * (n // 2) * (mk // 2) * 8
    planes = Guarded(pbytes, SENTINEL)
    assert planes.guard == 64 << 20
    L.check(lib.pls_onb_winograd_prepare(desc, planes.ptr, pbytes, L.stream_ptr()), "pls_onb_winograd_prepare")
    torch.cuda.synchronize()
    planes.assert_intact("pls_onb_winograd_prepare")
    planes.assert_written("pls_onb_winograd_prepare")
    assert int(lib.pls_onb_winograd_prepare(desc, planes.ptr, pbytes - 8, L.stream_ptr())) != OK
    qn = int(lib.pls_onb_step_workspace_bytes(desc, j, n))
    # the route takes chunks of at least 8192 paired rows: at N = 16384 all of them, whose seven right-hand planes need more
    # than the plain route's all-rows query (step_fixtures.wino_one_chunk_bytes, as tests/test_gpu_winograd.py)
    ws_bytes = wino_one_chunk_bytes(mk, n, j)
    assert ws_bytes > qn
    cols = torch.arange(0, j, 61)
    assert probe_winograd(P, gb, cost, u, ws_bytes=ws_bytes), "the Winograd route did not run"
    firsts = {}
    for energy in (True, False):
        for fill in FILLS:
            res = step_call(P, gb, cost, u, xi, fill, force_generic=True, energy=energy, ws_bytes=ws_bytes, wg=planes)
            what = f"winograd, energy {energy}, fill {fill}"
            contained(res, what)
            planes.assert_intact(what)
            if energy not in firsts:
                firsts[energy] = res
                print(f"winograd: workspace {ws_bytes} bytes, planes {pbytes} bytes, launches {sorted(set(res.tags))}")
                assert_exact(ex, res.out.matrix(), cols, energy=res.guards["energy_in"].f64() if energy else None, what=what)
            else:
                assert_same(firsts[energy], res, what)
            del res
    assert same_bits(firsts[True].out.matrix(), firsts[False].out.matrix()), "asking for the energies moved the Winograd step"
    del firsts
    # a smaller workspace -- the plain route's all-rows query -- is another route: the plain one, shown by planes it never reads
    assert not probe_winograd(P, gb, cost, u, ws_bytes=qn)
    res = step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=qn, wg=planes)
    contained(res, "plain route in its all-rows workspace")
    assert count(res.tags, "gemm_cost_deriv") == 1
    assert_exact(ex, res.out.matrix(), cols, energy=res.guards["energy_in"].f64(), what="plain route in its all-rows workspace")
    del res
    q128 = int(lib.pls_onb_step_workspace_bytes(desc, j, 128))
    refused(step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=q128 - 8, wg=planes), "winograd shape: one double short")


# -------------------------------------------------------------------------------------------------------------------------
# energies of the orthonormal basis, pls_cost_value
def fixture_energy(ex, e, what):
    """the exact fixtures' own assertion on an energy vector (step_fixtures.assert_exact's energy branch)"""
    assert_exact(ex, ex.step()[0], energy=e, what=what)


def onb_energy_call(P, gb, cost, u, fill, force_generic, ws_bytes):
    L = P.pkg._lib
    lib = L.load()
    j = u.shape[1]
    gaussian = gb._is_gaussian(cost, force_generic)
    if gaussian:
        gb.prepare_gaussian(cost.y_device())
    desc = gb._desc(with_gaussian=gaussian)
    res = Res()
    res.ws_bytes, res.entry, res.out, res.outputs, res.zeroed = ws_bytes, "pls_onb_energy", None, ["e"], []
    ws, e = Guarded(ws_bytes, fill), Guarded(8 * j, SENTINEL)
    res.guards = {"workspace": ws, "e": e}
    with L.Timeline(256) as tl:
        res.rc = lib.pls_onb_energy(desc, cost.desc(), cost.y_device().data_ptr(), u.data_ptr(), L.ld(u), j, e.ptr, int(force_generic),
                                    ws.ptr, ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    res.error = lib.pls_last_error().decode() if res.rc else ""
    res.tags = [name for name, _ in tl.records]
    res.keep = (desc, u)
    return res


@pytest.mark.parametrize("mk,n,j,force,chunk,tag,launches", [
    (30, 3000, 40, True, None, "small_rank_value", 1),     # the small-rank value kernel
    (200, 1500, 333, True, None, "gemm_cost_value", 1),    # the GEMM route, whole
    (200, 1500, 333, True, 512, "gemm_cost_value", 3),     # ... in chunks of 512 rows
    (100, 300, 333, False, None, "gemm_cost_value", 1),    # the Gaussian fast path: ONE M_k x M_k x J contraction (same tag)
    (129, 300, 1100, False, None, "gemm_cost_value", 1)])
def test_onb_energy(P, mk, n, j, force, chunk, tag, launches):
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, _ = onb(P, mk, n, j)
    gaussian = not force
    if gaussian:
        gb.prepare_gaussian(cost.y_device())
    desc = gb._desc(with_gaussian=gaussian)
    query = int(lib.pls_onb_energy_workspace_bytes(desc, j, chunk or n))
    what = f"pls_onb_energy {mk}x{n}x{j}, generic {force}, chunk {chunk}"
    first = None
    for fill in FILLS:
        res = onb_energy_call(P, gb, cost, u, fill, force, query)
        contained(res, f"{what}, fill {fill}, launches {res.tags}")
        assert count(res.tags, tag) == launches and not ({"gemm_cost_value", "small_rank_value"} - {tag}) & set(res.tags), res.tags
        if first is None:
            first = res
            print(f"{what}: workspace {query} bytes, launches {sorted(set(res.tags))}")
            fixture_energy(ex, res.guards["e"].f64(), what)
        else:
            assert_same(first, res, what)
    # the plain need: two partial rows of the cost value; cdiv(mk, 64) of the fast path's 64-row tiles
    need = (cdiv(mk, 64) if gaussian else 2) * j * 8
    refused(onb_energy_call(P, gb, cost, u, NAN, force, need - 8), f"{what}: one double short of {need} bytes")


@pytest.mark.parametrize("mk,n,j", [(100, 300, 333), (30, 3000, 40)])
def test_onb_prior_energy(P, mk, n, j):
    """outputs only: e(J) behind guards, with and without the cost vector"""
    L = P.pkg._lib
    lib = L.load()
    ex, gb, _, u, _ = onb(P, mk, n, j)
    c = torch.arange(j, dtype=F64) - 7.0
    prior = 0.5 * (ex.u * ex.u / ex.lam[:, None]).sum(0)
    for cost_vec, want in ((c.cuda(), c + prior), (None, prior)):
        e = Guarded(8 * j, SENTINEL)
        L.check(lib.pls_onb_prior_energy(gb._desc(), u.data_ptr(), L.ld(u), j, L.ptr(cost_vec), e.ptr, L.stream_ptr()), "pls_onb_prior_energy")
        torch.cuda.synchronize()
        e.assert_intact("pls_onb_prior_energy")
        e.assert_written("pls_onb_prior_energy")
        assert torch.equal(e.f64().cpu(), want), "pls_onb_prior_energy (every term is exact on these inputs)"


@pytest.mark.parametrize("n,j", [(130, 70), (1000, 8)])
def test_cost_value(P, n, j):
    """integer F and y, variance 1/4: every term 2 (f - y)^2 and every partial sum an integer"""
    L = P.pkg._lib
    lib = L.load()
    g = torch.Generator().manual_seed(n + j)
    f_host = torch.randint(-9, 10, (n, j), generator=g).double()
    y = torch.randint(-8, 9, (n,), generator=g).double()
    cost = P.costs.GaussianCost(0.25, y, P.links.IdentityLinkFunction())
    f = padded(f_host)
    want = (2 * (f_host - y[:, None]) ** 2).sum(0)
    need = int(lib.pls_cost_value_workspace_bytes(n, j))
    assert need > 0
    first = None
    for fill in FILLS:
        ws, c = Guarded(need, fill), Guarded(8 * j, SENTINEL)
        rc = lib.pls_cost_value(cost.desc(), f.data_ptr(), L.ld(f), cost.y_device().data_ptr(), n, j, c.ptr, ws.ptr, need, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == OK, lib.pls_last_error()
        for gd, name in ((ws, "workspace"), (c, "c")):
            gd.assert_intact(f"pls_cost_value {n}x{j}: {name}")
        c.assert_written("pls_cost_value")
        if first is None:
            first = c
            print(f"pls_cost_value {n}x{j}: workspace {need} bytes")
            assert torch.equal(c.f64().cpu(), want), "pls_cost_value on integers"
        else:
            assert same_bits(first.f64(), c.f64()), f"pls_cost_value depends on what its workspace held (fill {fill})"
    ws, c = Guarded(need - 8, NAN), Guarded(8 * j, SENTINEL)
    rc = lib.pls_cost_value(cost.desc(), f.data_ptr(), L.ld(f), cost.y_device().data_ptr(), n, j, c.ptr, ws.ptr, need - 8, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == TOO_SMALL
    ws.assert_intact("pls_cost_value, short workspace")
    c.assert_intact("pls_cost_value, short workspace")
    assert (c.bits() == SENTINEL_BITS).all()


# -------------------------------------------------------------------------------------------------------------------------
# the inducing-point basis
_ipb = {}


def ipb(P, m, n, j, **kw):
    key = (m, n, j, tuple(sorted(kw.items())))
    if key not in _ipb:
        if len(_ipb) >= 3:
            _ipb.clear()
        ex = exact_ipb(m, n, j)
        gb = ex.basis(P, **kw)
        _ipb[key] = (ex, gb, ex.cost(P), padded(ex.u), P.basis.NoiseSpec(injected=padded(ex.e)))
    return _ipb[key]


def flags_zero(gb):
    sc = gb._chol.tri_scratch()
    return sc is None or bool((sc[: gb._chol.TRI_FLAG_BYTES // 8] == 0).all())


IPB_SHAPES = [(64, 300, 40), (200, 1500, 333)]


def fixed_size_call(P, name, args_of, ws_bytes, fill, outputs):
    """one call of a fixed-size entry: ``args_of(ws_ptr, ws_bytes, outs)`` -> the C arguments; ``outputs``: name -> Guarded"""
    L = P.pkg._lib
    lib = L.load()
    res = Res()
    res.ws_bytes, res.entry, res.out, res.zeroed = ws_bytes, name, None, []
    ws = Guarded(ws_bytes, fill)
    res.guards = {"workspace": ws, **outputs}
    res.outputs = list(outputs)
    with L.Timeline(256) as tl:
        res.rc = getattr(lib, name)(*args_of(ws.ptr, ws_bytes))
    torch.cuda.synchronize()
    res.error = lib.pls_last_error().decode() if res.rc else ""
    res.tags = [t for t, _ in tl.records]
    return res


def fixed_size_cell(P, name, make, need, what, expect):
    """containment, independence and size honesty of a fixed-size entry.  ``make()`` -> (args_of, outputs) with fresh guarded
    outputs; ``expect(outputs)`` asserts the values"""
    first = None
    for fill in FILLS:
        args_of, outs = make()
        res = fixed_size_call(P, name, args_of, need, fill, outs)
        contained(res, f"{what}, fill {fill}")
        if first is None:
            first = res
            print(f"{what}: workspace {need} bytes, launches {sorted(set(res.tags))}")
            expect(outs)
        else:
            assert_same(first, res, what)
    args_of, outs = make()
    res = fixed_size_call(P, name, args_of, need - 8, NAN, outs)
    refused(res, f"{what}: one double short")
    for name_, gd in outs.items():
        assert (gd.bits() == SENTINEL_BITS).all(), f"{what}: {name_} was written by a refused call"
    return first


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
def test_ipb_forward_update_and_prior_energy(P, m, n, j):
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, e_noise = ipb(P, m, n, j)
    st = L.stream_ptr()
    v = ex.solve(ex.u)

    def forward():
        f = GuardedMatrix(n, j, j + 2 + j % 2)
        return (lambda w, wb: (gb._desc(), u.data_ptr(), L.ld(u), j, f.ptr, f.ld, w, wb, st)), {"F": f}

    fixed_size_cell(P, "pls_ipb_forward", forward, m * j * 8, f"pls_ipb_forward {m}x{n}x{j}",
                    lambda o: torch.equal(o["F"].matrix().cpu(), ex.kzx.T @ v) or pytest.fail("pls_ipb_forward differs from k(X,Z) V"))
    g_host = (ex.kzx.T @ v - ex.y[:, None]) / 0.25
    g = padded(g_host)
    want, _ = ex.step()

    def update():
        du = GuardedMatrix(m, j, j + 2 + j % 2)
        return (lambda w, wb: (gb._desc(), u.data_ptr(), L.ld(u), g.data_ptr(), L.ld(g), j, EXACT_ETA, e_noise.desc(), du.ptr, du.ld, w,
                               wb, st)), {"dU": du}

    fixed_size_cell(P, "pls_ipb_particle_update", update, 4 * cdiv(m * j * 8, 256) * 256, f"pls_ipb_particle_update {m}x{n}x{j}",
                    lambda o: torch.equal(o["dU"].matrix().cpu(), want) or pytest.fail("pls_ipb_particle_update differs from the exact step"))
    c = torch.arange(j, dtype=F64)
    cd = c.cuda()
    e_want = c + 0.5 * m * (v * v).sum(0)

    def prior():
        e = Guarded(8 * j, SENTINEL)
        return (lambda w, wb: (gb._desc(), u.data_ptr(), L.ld(u), j, cd.data_ptr(), e.ptr, w, wb, st)), {"e": e}

    def check_prior(o):
        got = o["e"].f64().cpu()
        assert ((got - e_want).abs() / e_want.abs()).max().item() <= 1e-13  # (the exact fixtures' bar on an energy)

    fixed_size_cell(P, "pls_ipb_prior_energy", prior, m * j * 8, f"pls_ipb_prior_energy {m}x{n}x{j}", check_prior)
    assert flags_zero(gb)


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
def test_ipb_build_whitened(P, m, n, j):
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, _ = ipb(P, m, n, j)
    gb.prepare_gaussian(cost.y_device())  # B and c alone: the descriptor of the build call carries no Q
    g2 = copy.copy(gb)
    g2._Q = g2._Pt = None
    desc = g2._desc(with_gaussian=True)
    need = int(lib.pls_ipb_build_whitened_workspace_bytes(m))
    ldq = m + 2 + m % 2

    def make():
        q, ct = GuardedMatrix(m, m, ldq), Guarded(8 * (m + 1), SENTINEL)
        return (lambda w, wb: (desc, 4.0, q.ptr, ldq, ct.ptr, w, wb, L.stream_ptr())), {"Q": q, "ct": ct}

    def expect(o):
        assert torch.equal(o["Q"].matrix().cpu(), ex.q), "Q"
        assert torch.equal(o["ct"].f64()[:m].cpu(), ex.ct.flatten()), "ct"
        assert o["ct"].f64()[m].item() == float((ex.y * ex.y).sum()), "y^T y behind ct"

    fixed_size_cell(P, "pls_ipb_build_whitened", make, need, f"pls_ipb_build_whitened {m}", expect)
    assert flags_zero(gb)


def ipb_general_cells(P, ex, gb, cost, u, xi, what, route_whole, route_chunked, n, **kw):
    L = P.pkg._lib
    lib = L.load()
    j = u.shape[1]
    desc = gb._route(cost, j, True).head[0]
    q128, qc, qn = (int(lib.pls_ipb_step_workspace_bytes(desc, j, c)) for c in (128, 256, n))
    whole = cell(P, ex, gb, cost, u, xi, f"{what}: whole", route=route_whole, force_generic=True, sums=True, sums16=True, **kw)
    assert whole.ws_bytes == qn
    sums_follow(P, whole, what)
    bare = cell(P, ex, gb, cost, u, xi, f"{what}: whole, no energies", route=route_whole, force_generic=True, energy=False, **kw)
    assert same_bits(bare.out.matrix(), whole.out.matrix())
    part = cell(P, ex, gb, cost, u, xi, f"{what}: 256-row query", route=route_chunked(cdiv(n, 256)), force_generic=True, ws_bytes=qc, **kw)
    least = cell(P, ex, gb, cost, u, xi, f"{what}: 128-row query", route=route_chunked(cdiv(n, 128)), force_generic=True, ws_bytes=q128, **kw)
    for r in (part, least):
        assert same_bits(r.out.matrix(), whole.out.matrix()), f"{what}: the chunked step differs from the whole one"
    refused(step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=q128 - 8, **kw), f"{what}: one double short of the 128-row query")
    assert flags_zero(gb)


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
def test_ipb_step_general_route(P, m, n, j):
    """force_generic with the one-launch step switched off: at M = 64 the slab kernels of small_rank.h (whatever the chunk the
    workspace holds), at M = 200 the GEMM route whole and in chunks (n = 1500: 256-row chunks end with a short one)"""
    L = P.pkg._lib
    ex, gb, cost, u, xi = ipb(P, m, n, j, explicit_inverse=True)
    with option(P, L.OPT_SMALL_RANK_STEP, 0):
        if m <= 128:
            ipb_general_cells(P, ex, gb, cost, u, xi, f"ipb general {m}x{n}x{j}", is_slab_kernels, lambda chunks: is_slab_kernels, n)
        else:
            ipb_general_cells(P, ex, gb, cost, u, xi, f"ipb general {m}x{n}x{j}", is_general(1), is_general, n)
            with option(P, L.OPT_IPB_EXPLICIT_INVERSE, 1):
                cell(P, ex, gb, cost, u, xi, f"ipb general {m}x{n}x{j}, explicit inverse", route=is_general(1), force_generic=True)
            with option(P, L.OPT_SOLVE_MODE, 0):
                cell(P, ex, gb, cost, u, xi, f"ipb general {m}x{n}x{j}, substitution",
                     route=lambda t: (is_general(1)(t), "tri_solve" in t or pytest.fail(str(t))), force_generic=True)


def test_ipb_step_one_launch_route(P):
    """M = 64: V and the coloured noise in one launch (csrc/ipb_prep.h), then the one-launch step; counters from the caller and
    carved from the workspace"""
    L = P.pkg._lib
    lib = L.load()
    m, n, j = 64, 300, 40
    ex, gb, cost, u, xi = ipb(P, m, n, j)
    query = int(lib.pls_ipb_step_workspace_bytes(gb._desc(), j, n))

    def route(tags):
        assert tags == ["ipb_prep", "small_rank_step"], tags

    with option(P, L.OPT_SMALL_RANK_STEP, 2):
        first = None
        for sync in ("caller", None):
            for kw in (dict(sums16=True), dict(sums=True), dict(energy=False)):
                what = f"ipb one launch, step_sync {sync}, {kw}"
                res = cell(P, ex, gb, cost, u, xi, what, route=route, force_generic=True, step_sync=sync, **kw)
                assert res.ws_bytes == query
                if kw.get("energy", True):
                    sums_follow(P, res, what)
                first = first or res
                assert same_bits(res.out.matrix(), first.out.matrix())
        with option(P, L.OPT_IPB_PREP, 0):
            cell(P, ex, gb, cost, u, xi, "ipb one launch behind two products",
                 route=lambda t: ("small_rank_step" in t and "ipb_prep" not in t) or pytest.fail(str(t)), force_generic=True, sums16=True)
        q128 = int(lib.pls_ipb_step_workspace_bytes(gb._desc(), j, 128))
        refused(step_call(P, gb, cost, u, xi, NAN, force_generic=True, ws_bytes=q128 - 8), "ipb one launch: one double short of the 128-row query")
    assert flags_zero(gb)


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
def test_ipb_step_gaussian_routes(P, m, n, j):
    """Gaussian / identity through pls_ipb_step: the whitened route (forward solve + Q S: the one that delivers energies), the
    Pt two-launch route (no energies), the round-2 fast route of a descriptor without Q, the explicit-inverse option"""
    from test_gpu_exact_ipb import poisoned

    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, xi = ipb(P, m, n, j, explicit_inverse=True)
    gb._prepare_for(cost)
    q128, qn = (int(lib.pls_ipb_step_workspace_bytes(gb._desc(with_gaussian=True), j, c)) for c in (128, n))

    def no_drift_stream(tags):
        assert "gemm_cost_deriv" not in tags and not any(t.startswith("small_rank") for t in tags), tags

    def whitened_route(tags):  # the fused Q S / P U contraction with the update in its epilogue
        no_drift_stream(tags)
        assert "gemm_langevin_gaussian" in tags, tags

    def fast_route(tags):  # B V as a storing contraction, the update a launch of its own
        no_drift_stream(tags)
        assert "gemm_langevin_gaussian" not in tags and "gemm_store" in tags, tags

    what = f"ipb gaussian {m}x{n}x{j}"
    white = cell(P, ex, gb, cost, u, xi, f"{what}: whitened, energies", route=whitened_route, sums=True, sums16=True)
    assert white.ws_bytes == qn
    sums_follow(P, white, what)
    pt = cell(P, ex, gb, cost, u, xi, f"{what}: Pt route", route=whitened_route, energy=False)
    assert same_bits(pt.out.matrix(), white.out.matrix())
    # the tags cannot tell the Pt route from the Q route: the operand only one of them reads can (NaN in, NaN out)
    e = torch.empty(j, dtype=F64, device="cuda")
    assert poisoned(gb, "Pt").fused_step(cost, u, EXACT_ETA, noise=xi).isnan().any(), f"{what}: without energies the step did not read Pt"
    assert same_bits(poisoned(gb, "Pt").fused_step(cost, u, EXACT_ETA, noise=xi, input_energy=e), white.out.matrix()), \
        f"{what}: with energies the step read Pt"
    assert poisoned(gb, "Q").fused_step(cost, u, EXACT_ETA, noise=xi, input_energy=e).isnan().any(), f"{what}: with energies the step did not read Q"
    with option(P, L.OPT_IPB_STEP_OPERATOR, 0):
        cell(P, ex, gb, cost, u, xi, f"{what}: whitened through Q, no energies", route=whitened_route, energy=False)
        assert same_bits(poisoned(gb, "Pt").fused_step(cost, u, EXACT_ETA, noise=xi), white.out.matrix()), f"{what}: operator 0 read Pt"
    least = cell(P, ex, gb, cost, u, xi, f"{what}: whitened, 128-row query", route=whitened_route, ws_bytes=q128)
    assert_same(direct_only(white), direct_only(least), f"{what}: the 128-row workspace")
    refused(step_call(P, gb, cost, u, xi, NAN, ws_bytes=q128 - 8), f"{what}: one double short of the 128-row query")
    with option(P, L.OPT_IPB_EXPLICIT_INVERSE, 1):
        cell(P, ex, gb, cost, u, xi, f"{what}: explicit inverse", route=fast_route, sums=True)
        assert poisoned(gb, "W").fused_step(cost, u, EXACT_ETA, noise=xi).isnan().any(), f"{what}: the explicit-inverse option did not read W"
    plain = copy.copy(gb)
    plain.whitened = False
    plain._prepare_for(cost)
    cell(P, ex, plain, cost, u, xi, f"{what}: fast route without Q", route=fast_route, sums=True)
    cell(P, ex, plain, cost, u, xi, f"{what}: fast route without Q, 128-row query", route=fast_route, ws_bytes=q128)
    assert poisoned(plain, "B").fused_step(cost, u, EXACT_ETA, noise=xi).isnan().any(), f"{what}: the fast route did not read B"
    assert flags_zero(gb)


def ipb_energy_call(P, gb, cost, u, fill, force_generic, ws_bytes, whitened=False):
    L = P.pkg._lib
    lib = L.load()
    j = u.shape[1]
    gaussian = gb._is_gaussian(cost, force_generic)
    if gaussian:
        gb._prepare_for(cost)
    desc = gb._desc(with_gaussian=gaussian)
    e = Guarded(8 * j, SENTINEL)
    if whitened:
        return fixed_size_call(P, "pls_ipb_whitened_energy",
                               lambda w, wb: (desc, cost.desc(), u.data_ptr(), L.ld(u), j, e.ptr, w, wb, L.stream_ptr()), ws_bytes, fill, {"e": e})
    return fixed_size_call(P, "pls_ipb_energy",
                           lambda w, wb: (desc, cost.desc(), cost.y_device().data_ptr(), u.data_ptr(), L.ld(u), j, e.ptr, int(force_generic), w, wb,
                                          L.stream_ptr()), ws_bytes, fill, {"e": e})


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
@pytest.mark.parametrize("force", [True, False])
def test_ipb_energy(P, m, n, j, force):
    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, u, _ = ipb(P, m, n, j)
    gaussian = not force
    if gaussian:
        gb._prepare_for(cost)
    desc = gb._desc(with_gaussian=gaussian)
    what = f"pls_ipb_energy {m}x{n}x{j}, generic {force}"
    mj = cdiv(m * j * 8, 256) * 256
    for chunk in (n, 128):
        query = int(lib.pls_ipb_energy_workspace_bytes(desc, j, chunk))
        first = None
        for fill in FILLS:
            res = ipb_energy_call(P, gb, cost, u, fill, force, query)
            contained(res, f"{what}, {chunk}-row query, fill {fill}")
            if first is None:
                first = res
                print(f"{what}: {chunk}-row query {query} bytes, launches {sorted(set(res.tags))}")
                fixture_energy(ex, res.guards["e"].f64(), what)
            else:
                assert_same(first, res, what)
    # the plain need: V and two partial rows of the cost value; V and the m x j buffer of B V on the fast path
    need = 2 * mj if gaussian else mj + 2 * j * 8
    refused(ipb_energy_call(P, gb, cost, u, NAN, force, need - 8), f"{what}: one double short of {need} bytes")
    assert flags_zero(gb)


@pytest.mark.parametrize("m,n,j", IPB_SHAPES)
def test_ipb_whitened_step_and_energy(P, m, n, j):
    """pls_ipb_whitened_step / _blocks: direct, sums + sync, lagged + flush; pls_ipb_whitened_energy"""
    from test_gpu_exact_ipb import assert_whitened

    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, _, _ = ipb(P, m, n, j)
    gb._prepare_for(cost)
    s, xi = padded(ex.s), P.basis.NoiseSpec(injected=padded(ex.xi))
    query = int(lib.pls_ipb_whitened_workspace_bytes(gb._desc(with_gaussian=True), j))
    pbytes = int(lib.pls_energy_partials_bytes(m, j))
    what = f"whitened step {m}x{n}x{j}"

    def check(out, e):
        assert_whitened(ex, out, energy=e, what=what)

    plain = cell(P, ex, gb, cost, s, xi, f"{what}: no energies", route=is_fast, check=check, whitened=True, energy=False)
    assert plain.ws_bytes == 0
    direct = cell(P, ex, gb, cost, s, xi, f"{what}: direct", route=is_fast, check=check, whitened=True, sums=True, sums16=True)
    assert direct.ws_bytes == query
    sums_follow(P, direct, what)
    assert same_bits(direct.out.matrix(), plain.out.matrix())
    fused = cell(P, ex, gb, cost, s, xi, f"{what}: sums + sync", route=is_fast, check=check, whitened=True, sums=True, esync=True)
    assert fused.tags == ["gemm_langevin_gaussian"], fused.tags
    assert same_bits(fused.guards["energy_in"].f64(), direct.guards["energy_in"].f64())
    assert same_bits(fused.guards["energy_sums"].f64(), direct.guards["energy_sums"].f64())
    for fill in FILLS:
        bufs = [Guarded(pbytes, fill), Guarded(pbytes, fill)]
        a = step_call(P, gb, cost, s, xi, fill, whitened=True, lag=dict(out=bufs[0]))
        contained(a, f"{what}: lagged, first launch")
        b = step_call(P, gb, cost, s, xi, fill, whitened=True, lag=dict(out=bufs[1], prev=bufs[0]))
        contained(b, f"{what}: lagged, second launch")
        f = step_call(P, gb, cost, s, xi, fill, whitened=True, lag=dict(prev=bufs[1], flush=True))
        contained(f, f"{what}: flush")
        for r in (a, b):
            assert same_bits(r.out.matrix(), plain.out.matrix())
        for r in (b, f):
            assert same_bits(r.guards["energy_prev"].f64(), direct.guards["energy_in"].f64()), f"{what}: lagged energies, fill {fill}"
            assert same_bits(r.guards["energy_sums_prev"].f64(), direct.guards["energy_sums"].f64()), f"{what}: lagged sums"
    small = step_call(P, gb, cost, s, xi, NAN, whitened=True, ws_bytes=query - 8)
    if small.rc == OK:  # (a launch of 64-row tiles leaves cdiv(m, 64) partial rows: see test_onb_fast_path)
        assert cdiv(m, 64) < 2 * cdiv(m, 128)
        contained(small, f"{what}: one double short of the documented size")
        assert_same(direct_only(direct), direct_only(small), f"{what}: short workspace")
        small = step_call(P, gb, cost, s, xi, NAN, whitened=True, ws_bytes=cdiv(m, 64) * j * 8 - 8)
    refused(small, f"{what}: one double short")
    # pls_ipb_whitened_energy: the same workspace query
    first = None
    for fill in FILLS:
        res = ipb_energy_call(P, gb, cost, s, fill, False, query, whitened=True)
        contained(res, f"pls_ipb_whitened_energy, fill {fill}")
        if first is None:
            first = res
            assert_whitened(ex, plain.out.matrix(), energy=res.guards["e"].f64(), what="pls_ipb_whitened_energy")
        else:
            assert_same(first, res, "pls_ipb_whitened_energy")
    refused(ipb_energy_call(P, gb, cost, s, NAN, False, cdiv(m, 64) * j * 8 - 8, whitened=True), "pls_ipb_whitened_energy: one double short")


@pytest.mark.parametrize("n,m,j", [(50, 1, 8), (333, 16, 37)])
def test_ipb_whitened_generic_step(P, n, m, j):
    from test_gpu_exact_ipb import assert_whitened

    L = P.pkg._lib
    lib = L.load()
    ex, gb, cost, _, _ = ipb(P, m, n, j)
    assert gb.whitened_generic_applies(cost, j, force_generic=True)
    s, xi = padded(ex.s), P.basis.NoiseSpec(injected=padded(ex.xi))
    query = int(lib.pls_ipb_whitened_generic_workspace_bytes(gb._desc(), j))
    what = f"whitened generic {n}x{m}x{j}"

    def check(out, e):
        assert_whitened(ex, out, energy=e, what=what)

    first = None
    for sync in ("caller", None):
        for kw in (dict(sums16=True), dict(sums=True), dict(energy=False)):
            res = cell(P, ex, gb, cost, s, xi, f"{what}, step_sync {sync}, {kw}", route=is_one_launch, check=check, whitened=True,
                       force_generic=True, step_sync=sync, **kw)
            assert res.ws_bytes == query
            if kw.get("energy", True):
                sums_follow(P, res, what)
            first = first or res
            assert same_bits(res.out.matrix(), first.out.matrix())
    # counters carved from the workspace and the sums asked for: the layout is the query, one double less is refused
    refused(step_call(P, gb, cost, s, xi, NAN, whitened=True, force_generic=True, sums=True, ws_bytes=query - 8), f"{what}: one double short")


# -------------------------------------------------------------------------------------------------------------------------
# the other workspace-taking entries
@pytest.mark.parametrize("m,j", [(65, 33), (200, 257)])
@pytest.mark.parametrize("inverse", [True, False])
def test_chol_solve_ws(P, m, j, inverse):
    """with the inverse factor: two triangular products through the workspace; one double less: the substitution kernel, the
    same (exact) solve; without the inverse factor the workspace is not used at all"""
    from projected_langevin_sampling_amd import _chol

    L = P.pkg._lib
    lib = L.load()
    ex = exact_ipb(m, 16, j)
    f = _chol.cholesky_factor(ex.kzz.cuda())
    if inverse:
        f.build_inverse()
    u = padded(ex.u)
    want = ex.solve(ex.u)
    need = int(lib.pls_chol_solve_workspace_bytes(m, j))
    assert need == m * j * 8
    for ws_bytes, substitution in ((need, not inverse), (need - 8, True)):
        first = None
        for fill in FILLS:
            v = GuardedMatrix(m, j, j + 2 + j % 2)
            res = fixed_size_call(P, "pls_chol_solve_ws", lambda w, wb: (f.desc(), u.data_ptr(), L.ld(u), j, v.ptr, v.ld, w, wb, L.stream_ptr()),
                                  ws_bytes, fill, {"V": v})
            what = f"pls_chol_solve_ws {m}x{j}, inverse factor {inverse}, workspace {ws_bytes}, fill {fill}, launches {res.tags}"
            contained(res, what)
            assert ("tri_solve" in res.tags) == substitution, what
            if first is None:
                first = res
                assert torch.equal(v.matrix().cpu(), want), what
            else:
                assert_same(first, res, what)
    sc = f.tri_scratch()
    assert sc is None or bool((sc[: f.TRI_FLAG_BYTES // 8] == 0).all())


@pytest.mark.parametrize("n,m,d", [(200, 12, 2), (1000, 40, 3)])
@pytest.mark.parametrize("kind", ["rbf", "periodic"])
def test_select_inducing(P, n, m, d, kind):
    """n off the 256 grid; the byte-sized `chosen` region sits mid-layout.  The expected indices: the same call in an ordinary
    zero-filled buffer twice the size"""
    L = P.pkg._lib
    lib = L.load()
    g = torch.Generator().manual_seed(n + m + d)
    x = torch.rand(n, d, generator=g, dtype=F64).cuda()
    if kind == "rbf":
        k, params = L.KERNEL_RBF_ARD, (0.3 + torch.rand(d, generator=g, dtype=F64)).cuda()
    else:
        k, params = L.KERNEL_PERIODIC, torch.cat([0.5 + torch.rand(d, generator=g, dtype=F64), 0.7 + torch.rand(d, generator=g, dtype=F64)]).cuda()
    need = int(lib.pls_select_inducing_workspace_bytes(n, m))
    st = L.stream_ptr()
    ref_ws = torch.zeros(2 * need // 8 + 1, dtype=F64, device="cuda")
    ref_idx, ref_count = torch.full((m,), -1, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    L.check(lib.pls_select_inducing_conditional_variance(k, x.data_ptr(), n, d, params.data_ptr(), 1.3, m, 1e-12, -1.0, ref_idx.data_ptr(),
                                                         ref_count.data_ptr(), ref_ws.data_ptr(), need, st), "select_inducing")
    assert int(ref_count.item()) == m and len(set(ref_idx.tolist())) == m and 0 <= int(ref_idx.min()) and int(ref_idx.max()) < n

    def make():
        idx, cnt = Guarded(8 * m, SENTINEL), Guarded(8, SENTINEL)
        return (lambda w, wb: (k, x.data_ptr(), n, d, params.data_ptr(), 1.3, m, 1e-12, -1.0, idx.ptr, cnt.ptr, w, wb, st)), \
            {"indices": idx, "count": cnt}

    def expect(o):
        assert torch.equal(o["indices"].bits(), ref_idx) and torch.equal(o["count"].bits(), ref_count)

    fixed_size_cell(P, "pls_select_inducing_conditional_variance", make, need, f"select_inducing {n}x{m}x{d} {kind}", expect)


GP_KINDS = ["rbf", "rq", "periodic", "trend_seasonal"]


def gp_params(L, kind, d, g):
    def pos(k, lo):
        return lo + torch.rand(k, generator=g, dtype=F64)

    if kind == "rbf":
        return L.KERNEL_RBF_ARD, pos(d, 0.5)
    if kind == "rq":
        return L.KERNEL_RQ, torch.cat([pos(d, 0.5), pos(1, 0.8)])
    if kind == "periodic":
        return L.KERNEL_PERIODIC, torch.cat([pos(d, 0.5), pos(d, 0.7)])
    return L.KERNEL_TREND_SEASONAL, torch.cat([pos(d, 1.0), pos(d, 0.8), pos(d, 0.5), pos(d, 0.7), pos(1, 0.4)])


@pytest.mark.parametrize("n,d", [(65, 3), (130, 8)])
@pytest.mark.parametrize("kind", GP_KINDS)
def test_gp_mll_grad_and_classes(P, n, d, kind):
    """one kind per layout width; the expected values: the same evaluation through tests/base_kernel_calls.gp_mll (which the
    per-family files hold to their closed forms), bit for bit.  The guard behind the workspace is what that wrapper lacks."""
    L = P.pkg._lib
    lib = L.load()
    g = torch.Generator().manual_seed(n + d)
    k, params_host = gp_params(L, kind, d, g)
    x, y = torch.rand(n, d, generator=g, dtype=F64), torch.randn(n, generator=g, dtype=F64)
    params = params_host.cuda()
    width = 4 + d + L.kernel_shape_params(k, d)
    assert params.numel() == width - 4
    s, noise, mean = 1.3, 0.2, 0.1
    want, info, rc = bkc.gp_mll(P, k, x, y, params, s, noise, mean, fill=0.0)
    assert rc == OK and info == 0 and torch.isfinite(want).all()
    xd, yd = x.cuda(), y.cuda()
    need = int(lib.pls_gp_mll_workspace_bytes_kind(k, n, d))
    st = L.stream_ptr()

    def make():
        out, inf = Guarded(8 * width, SENTINEL), Guarded(4, 0.0)
        inf.view(torch.int32).fill_(-7)
        return (lambda w, wb: (k, xd.data_ptr(), n, d, params.data_ptr(), s, noise, mean, 0.0, yd.data_ptr(), out.ptr, inf.ptr, w, wb, st)), \
            {"out": out, "info": inf}

    def expect(o):
        assert same_bits(o["out"].f64().cpu(), want), f"pls_gp_mll_grad {kind}"
        assert int(o["info"].view(torch.int32).item()) == 0

    first = None
    for fill in FILLS:
        args_of, outs = make()
        res = fixed_size_call(P, "pls_gp_mll_grad", args_of, need, fill, outs)
        res.outputs = ["out"]
        contained(res, f"pls_gp_mll_grad {kind} {n}x{d}, fill {fill}")
        if first is None:
            first = res
            print(f"pls_gp_mll_grad {kind} {n}x{d}: workspace {need} bytes")
        expect(outs)
    args_of, outs = make()
    res = fixed_size_call(P, "pls_gp_mll_grad", args_of, need - 8, NAN, outs)
    refused(res, f"pls_gp_mll_grad {kind}: one double short")
    assert (outs["out"].bits() == SENTINEL_BITS).all() and int(outs["info"].view(torch.int32).item()) == -7
    # two classes with class 1 = class 0's parameters: both rows the single evaluation, in the workspace of one
    classes = 2
    assert int(lib.pls_gp_mll_classes_workspace_bytes_kind(k, n, d, classes)) == need
    cparams = torch.stack([params_host, params_host]).cuda().contiguous()
    ys = torch.stack([y, y]).cuda().contiguous()
    host = (ctypes.c_double * classes)
    sc, nz, mn = host(s, s), host(noise, noise), host(mean, mean)
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for fill in FILLS:
        out, inf = Guarded(8 * width * classes, SENTINEL), Guarded(4 * classes, 0.0)
        res = fixed_size_call(P, "pls_gp_mll_grad_classes",
                              lambda w, wb: (k, xd.data_ptr(), n, d, classes, cparams.data_ptr(), addr(sc), addr(nz), addr(mn), None, n,
                                             ys.data_ptr(), n, 0.0, out.ptr, inf.ptr, w, wb, st), need, fill, {"out": out, "info": inf})
        res.outputs = ["out"]
        contained(res, f"pls_gp_mll_grad_classes {kind} {n}x{d}, fill {fill}")
        for c in range(classes):
            assert same_bits(out.f64()[c * width:(c + 1) * width].cpu(), want), f"pls_gp_mll_grad_classes {kind}: class {c}"
        assert inf.view(torch.int32).tolist() == [0, 0]
    out, inf = Guarded(8 * width * classes, SENTINEL), Guarded(4 * classes, 0.0)
    res = fixed_size_call(P, "pls_gp_mll_grad_classes",
                          lambda w, wb: (k, xd.data_ptr(), n, d, classes, cparams.data_ptr(), addr(sc), addr(nz), addr(mn), None, n,
                                         ys.data_ptr(), n, 0.0, out.ptr, inf.ptr, w, wb, st), need - 8, NAN, {"out": out, "info": inf})
    refused(res, f"pls_gp_mll_grad_classes {kind}: one double short")


@pytest.mark.parametrize("likelihood", ["gaussian", "lik_gaussian", "bernoulli", "student4.5"])
def test_svgp_entries(P, likelihood):
    """(n, m, batch) = (150, 17, 64): pls_svgp_elbo_grad on a batch and pls_svgp_sgd_epoch over a shuffled permutation (ragged
    last batch) -- "gaussian" --, and their _lik_ forms with the Gaussian, Bernoulli and Student-t likelihoods.  Expected values
    of an evaluation: the fsum helper (svgp_truth / svgp_quadrature_truth evaluate_inputs) under the bar of the SVGP files' own
    _check, and the bits of the same call in the ordinary oversized workspace of their Dev; of an epoch: the bits of the same
    epoch in that ordinary workspace (which tests/test_gpu_svgp*.py hold to its replay)."""
    import test_gpu_svgp
    import test_gpu_svgp_quadrature as quad

    n, m, batch = 150, 17, 64
    old_entry = likelihood == "gaussian"
    lik = "gaussian" if likelihood.endswith("gaussian") else likelihood
    inp = svgp_truth.make_inputs(840000 + m, n, m, batch)
    if lik != "gaussian":
        inp = svgp_quadrature_truth.with_targets(lik, inp)
    L = P.pkg._lib
    lib = L.load()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n + m)).cuda()
    idx = inp["idx"].cuda()
    need_grad, need_epoch = int(lib.pls_svgp_workspace_bytes(batch, m, batch)), int(lib.pls_svgp_workspace_bytes(n, m, batch))
    st = L.stream_ptr()
    grad_name, epoch_name = ("pls_svgp_elbo_grad", "pls_svgp_sgd_epoch") if old_entry else ("pls_svgp_lik_elbo_grad", "pls_svgp_lik_sgd_epoch")

    def fresh():
        dev = quad.Dev(inp, lik)
        return dev, ctypes.byref(dev.desc.base) if old_entry else ctypes.byref(dev.desc)

    def grad_args(dev, dref, out, gm, gl):
        return lambda w, wb: (dref, dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls, dev.scalars.data_ptr(), idx.data_ptr(), batch, out.ptr,
                              gm.ptr, gl.ptr, gl.ld, w, wb, st)

    def epoch_args(dev, dref, loss):
        return lambda w, wb: (dref, dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls, dev.scalars.data_ptr(), perm.data_ptr(), batch, 0.05, 3,
                              loss.ptr, w, wb, st)

    def grad_outputs():
        return Guarded(8 * 5, SENTINEL), Guarded(8 * m, SENTINEL), GuardedMatrix(m, m, m + 1)

    def state(dev):
        return tuple(t.view(torch.int64).clone() for t in (dev.mean, dev.ls_buf, dev.scalars))

    # what the outputs must be: the fsum helper under the SVGP files' bar, and the bits of the call in an ordinary workspace
    dev, _ = fresh()
    ordinary = dev.vector(*dev.evaluate(old_entry=old_entry))
    if lik == "gaussian":
        want, scale = svgp_truth.evaluate_inputs(inp), svgp_truth.evaluate_inputs(inp, majorant=True)
    else:
        want, scale = svgp_quadrature_truth.evaluate_inputs(lik, inp), svgp_quadrature_truth.evaluate_inputs(lik, inp, scale=True)
    for fill in FILLS:
        dev, dref = fresh()
        out, gm, gl = grad_outputs()
        res = fixed_size_call(P, grad_name, grad_args(dev, dref, out, gm, gl), need_grad, fill, {"out": out, "grad_m": gm, "grad_L": gl})
        res.outputs = ["out", "grad_m"]
        what = f"{grad_name} {likelihood}, fill {fill}"
        contained(res, what)
        k, l = dev.tril
        assert (gl.matrix(torch.int64)[k, l] != SENTINEL_BITS).all(), f"{what}: grad_L not written below the diagonal"
        upper = torch.triu(torch.ones(m, m, dtype=torch.bool, device="cuda"), diagonal=1)
        assert (gl.matrix(torch.int64)[upper] == SENTINEL_BITS).all(), f"{what}: grad_L written above the diagonal"
        got = dev.vector(out.f64(), gm.f64(), gl.matrix())
        assert np.array_equal(got.view(np.int64), ordinary.view(np.int64)), f"{what}: not the bits of the call in an ordinary workspace"
        if fill != fill:
            print(f"{grad_name} {likelihood}: workspace {need_grad} bytes, launches {sorted(set(res.tags))}")
            if lik == "gaussian":
                test_gpu_svgp._check(what, got, want, np.zeros_like(want), scale, m, batch)
            else:
                quad._check(what, lik, got, want, np.zeros_like(want), scale, m, batch)
    dev, dref = fresh()
    out, gm, gl = grad_outputs()
    refused(fixed_size_call(P, grad_name, grad_args(dev, dref, out, gm, gl), need_grad - 8, NAN, {"out": out, "grad_m": gm, "grad_L": gl}),
            f"{grad_name} {likelihood}: one double short")
    # the epoch in the Dev's ordinary workspace (the bytes of a full batch and two doubles more, NaN-filled)
    dev, dref = fresh()
    loss_ordinary = torch.full((1,), NAN, dtype=F64, device="cuda")
    L.check(getattr(lib, epoch_name)(dref, dev.mean.data_ptr(), dev.ls.data_ptr(), dev.ldls, dev.scalars.data_ptr(), perm.data_ptr(), batch, 0.05,
                                     3, loss_ordinary.data_ptr(), dev.ws.data_ptr(), dev.ws_bytes, st), epoch_name)
    torch.cuda.synchronize()
    assert dev.ws_bytes > need_epoch and torch.isfinite(loss_ordinary).all()
    ordinary = (loss_ordinary.view(torch.int64).clone(),) + state(dev)
    start_state = state(fresh()[0])
    assert not torch.equal(ordinary[1], start_state[0]) and not torch.equal(ordinary[2], start_state[1]), "the epoch did not move the state"
    for fill in FILLS:
        dev, dref = fresh()
        loss = Guarded(8, SENTINEL)
        res = fixed_size_call(P, epoch_name, epoch_args(dev, dref, loss), need_epoch, fill, {"loss": loss})
        what = f"{epoch_name} {likelihood}, fill {fill}"
        contained(res, what)
        got = (loss.bits().clone(),) + state(dev)
        assert all(torch.equal(a, b) for a, b in zip(ordinary, got)), f"{what}: not the bits of the epoch in an ordinary workspace"
    print(f"{epoch_name} {likelihood}: workspace {need_epoch} bytes")
    dev, dref = fresh()
    before = state(dev)
    loss = Guarded(8, SENTINEL)
    refused(fixed_size_call(P, epoch_name, epoch_args(dev, dref, loss), need_epoch - 8, NAN, {"loss": loss}), f"{epoch_name}: one double short")
    assert all(torch.equal(a, b) for a, b in zip(before, state(dev))), "a refused epoch moved the state"
