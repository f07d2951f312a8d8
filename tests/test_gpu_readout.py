"""GPU: the read-out side -- the numbers a user reads off the particles -- pinned to arithmetic.

  energy sums      pls_chunk_sums, pls_sums16 and pls_block_means against the documented orders restated on the host
                   (readout_truth), bit for bit, and against exact sums inside the bounds the orders give
  row power sums   pls_row_power_sums: power 1 bit for bit against its restated order; power 2 bit for bit where every product
                   and partial sum is exact, inside its bound on log-spread inputs (whether the compiler contracts s += v * v is
                   not the kernel's business)
  quantiles        exact ranks: the k-th order statistic itself, through the LDS sort and through the radix selection
  guard bands      each of the six entries once at a ragged shape: nothing outside the output written, every entry written
  prediction       V~^T k(Z, x) and the predicted samples per element, against long-double contractions with bounds from the
                   contraction lengths
  link transform   a tall matrix (the grid-stride loop over rows) against its one-row calls, bit for bit

Largest array: 131 329 doubles; largest contraction 200 x 1030 x 300."""
import math

import numpy as np
import pytest
import torch

import readout_truth as T
from test_gpu_parity import P, _f64_default, build_onb, make_problem  # noqa: F401  (fixtures)
from workspace_guards import SENTINEL, SENTINEL_BITS, Guarded, GuardedMatrix

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
OK = 0
U = 2.0 ** -53
SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 4097, 8192, 131072 + 257]
BLOCK_COLS = [1, 16, 96, 255, 256, 257, 1000]
cdiv = T.cdiv


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# energy sums
def vector_call(P, name, e, n_out):
    """pls_chunk_sums / pls_sums16 on the device vector ``e`` -> host array"""
    L = P.pkg._lib
    out = torch.full((n_out,), NAN, dtype=F64, device="cuda")
    L.check(getattr(L.load(), name)(e.data_ptr(), e.numel(), out.data_ptr(), L.stream_ptr()), name)
    return host(out)


@pytest.mark.parametrize("j", SIZES)
def test_energy_sums_follow_their_documented_orders(P, j):
    """131 329 columns are one block of 514 chunks: block_means_kernel's outer loop runs twice"""
    from projected_langevin_sampling_amd import _ops, trainers

    e = T.log_spread(j, seed=j)
    ed, ex = dev(e), T.ExactVector(e)
    chunk = vector_call(P, "pls_chunk_sums", ed, cdiv(j, 256))
    assert T.same_bits(chunk, T.chunk_sums(e)), "pls_chunk_sums differs from chunk256_sum's documented order"
    s16 = vector_call(P, "pls_sums16", ed, cdiv(j, 16))
    assert T.same_bits(s16, T.sums16(e)), "pls_sums16 differs from sixteen ascending adds"
    mean = _ops.block_means(ed)
    assert mean.shape == (1,) and T.same_bits(host(mean), T.block_means(e)), "pls_block_means over the whole vector"
    worst = {"chunk sums": max(T.chunk_sum_errors(chunk, e, ex)), "sums16": max(T.sums16_errors(s16, e, ex)),
             "mean": max(T.block_mean_errors(host(mean), e, ex=ex))}
    for bc in BLOCK_COLS:
        got = host(_ops.block_means(ed, bc))
        assert got.shape == (cdiv(j, bc),)
        want = T.block_means(e, bc)
        diff = np.nonzero(T.bits(got) != T.bits(want))[0]
        assert diff.size == 0, f"pls_block_means, blocks of {bc}: {diff.size} of {got.size} blocks differ, first {diff[0]}"
        worst[f"means of {bc}"] = max(T.block_mean_errors(got, e, bc, ex))
    print(f"j = {j}: |error| / bound against the exact sums {worst}")
    assert max(worst.values()) <= 1.0, worst
    # the host side of the training loops: the chunk sums as they arrive (an array), and as a list
    for sums in (chunk, chunk.tolist()):
        assert T.same_bits(trainers.mean_from_chunk_sums(sums, j), mean.item()), "mean_from_chunk_sums differs from pls_block_means"


def test_block_means_into_pinned_host_memory(P):
    """out_ptr: the training loops' slot of pinned host memory, read after a stream synchronise"""
    from projected_langevin_sampling_amd import _ops

    j, bc = 513, 96
    e = T.log_spread(j, seed=77)
    slot = torch.full((cdiv(j, bc) + 2,), SENTINEL_BITS, dtype=torch.int64).view(F64).pin_memory()
    assert _ops.block_means(dev(e), bc, out_ptr=slot.data_ptr()) is None
    torch.cuda.current_stream().synchronize()
    got = slot.numpy()
    assert T.same_bits(got[:-2], T.block_means(e, bc))
    assert (T.bits(got[-2:]) == SENTINEL_BITS).all(), "a store behind the last block"


def test_energy_sums_of_no_columns_write_nothing(P):
    L = P.pkg._lib
    lib = L.load()
    e = torch.ones(1, dtype=F64, device="cuda")
    for name, args in (("pls_block_means", (0, 1)), ("pls_block_means", (0, 256)), ("pls_chunk_sums", (0,)), ("pls_sums16", (0,))):
        out = Guarded(8, SENTINEL)
        assert getattr(lib, name)(e.data_ptr(), *args, out.ptr, L.stream_ptr()) == OK, lib.pls_last_error()
        torch.cuda.synchronize()
        out.assert_intact(f"{name}, j = 0")
        assert (out.bits() == SENTINEL_BITS).all(), f"{name} wrote an output for j = 0"


# ---------------------------------------------------------------------------------------------------------------------------
# pls_row_power_sums
COLS = [0, 1, 2, 255, 256, 257, 511, 513, 8193, 70001]
# every (rows, cols) whose padded matrix stays within the largest array of this file, 131 329 doubles
ROW_SHAPES = [(r, c) for r in (1, 3, 300) for c in COLS if r * (c + 3) <= 131072 + 257]


def laid_out(x, pad):
    """(flat device buffer, lds): the host matrix with lds = cols + pad, NaN in the padding (never a NULL pointer)"""
    rows, cols = x.shape
    lds = cols + pad
    buf = torch.full((max(rows * lds, 1),), NAN, dtype=F64, device="cuda")
    if cols:
        buf.as_strided((rows, cols), (lds, 1)).copy_(torch.from_numpy(x))
    return buf, lds


def rps(P, laid, rows, cols, power, shift=None):
    L = P.pkg._lib
    buf, lds = laid
    out = torch.full((rows,), NAN, dtype=F64, device="cuda")
    L.check(L.load().pls_row_power_sums(buf.data_ptr(), lds, rows, cols, L.ptr(shift), power, out.data_ptr(), L.stream_ptr()),
            "pls_row_power_sums")
    return host(out)


def dyadic_rows(rows, cols, seed):
    """(x, mean, sum of squared deviations): x = (m + d) 2^-7 with integers |d| <= 1024 that cancel in every row, so the row mean
    is m 2^-7 exactly and every deviation, square and partial sum (< 70001 x 2^20) is exact in any order"""
    rng = np.random.default_rng(seed)
    x, mean, sq = np.zeros((rows, cols)), np.zeros(rows), np.zeros(rows)
    for r in range(rows):
        half = rng.integers(-1024, 1025, size=cols // 2)
        d = np.concatenate([half, -half, np.zeros(cols % 2, dtype=np.int64)])
        rng.shuffle(d)
        m = int(rng.integers(-100, 101))
        x[r], mean[r], sq[r] = (m + d) * 2.0 ** -7, m * 2.0 ** -7, float((d * d).sum()) * 2.0 ** -14
    return x, mean, sq


@pytest.mark.parametrize("rows,cols", ROW_SHAPES)
def test_row_power_sums(P, rows, cols):
    """more than 256 columns: the strided loop takes further trips; lds = cols + 3 with NaN behind every row"""
    x = T.log_spread((rows, cols), seed=1000 * rows + cols)
    shift = 0.5 + 3.0 * np.random.default_rng(rows + cols).standard_normal(rows)  # (no row without a shift)
    shift_d = dev(shift)
    xd, md, sqd = dyadic_rows(rows, cols, seed=cols + rows)
    want1, want1s = T.row_power_sums(x, 1), T.row_power_sums(x, 1, shift)
    first = None
    for pad in (0, 3):
        lay, lay_d = laid_out(x, pad), laid_out(xd, pad)
        p1 = rps(P, lay, rows, cols, 1)
        mean = dev(p1) / cols if cols else torch.zeros(rows, dtype=F64, device="cuda")  # (the device's own mean)
        got = {"sum": p1, "shifted sum": rps(P, lay, rows, cols, 1, shift_d), "squares": rps(P, lay, rows, cols, 2, mean),
               "dyadic sum": rps(P, lay_d, rows, cols, 1)}
        mean_d = dev(got["dyadic sum"]) / cols if cols else torch.zeros(rows, dtype=F64, device="cuda")
        got["dyadic squares"] = rps(P, lay_d, rows, cols, 2, mean_d)
        what = f"{rows} x {cols}, lds {lay[1]}"
        assert T.same_bits(got["sum"], want1), f"{what}: power 1 differs from the documented order"
        assert T.same_bits(got["shifted sum"], want1s), f"{what}: power 1 about a shift differs from the documented order"
        if cols:
            assert np.array_equal(host(mean_d), md), f"{what}: the mean of a row whose sum is exact"
        assert T.same_bits(got["dyadic squares"], sqd), f"{what}: power 2 on exact products and sums"
        again = {"sum": rps(P, lay, rows, cols, 1), "squares": rps(P, lay, rows, cols, 2, mean)}
        assert all(T.same_bits(again[k], got[k]) for k in again), f"{what}: two runs differ"
        if first is None:
            first = got
            mean_h = host(mean)
            worst = {"sum": max(T.row_power_sum_errors(got["sum"], x, 1)),
                     "shifted sum": max(T.row_power_sum_errors(got["shifted sum"], x, 1, shift)),
                     "squares": max(T.row_power_sum_errors(got["squares"], x, 2, mean_h))}
            print(f"{what}: |error| / bound against the exact sums {worst}")
            assert max(worst.values()) <= 1.0, worst
        else:
            assert all(T.same_bits(first[k], got[k]) for k in got), f"{what}: the padded layout changed the sums"


def test_gaussian_predict_is_the_two_row_reductions(P):
    """GaussianCost.predict at the benchmark's particle count: mean = row sums / J, variance = squared deviations / (J - 1)"""
    from projected_langevin_sampling_amd import _ops

    rows, j = 7, 8193
    rng = np.random.default_rng(5)
    s_host = 1.5 + 2.0 * rng.standard_normal((rows, j))
    s = dev(s_host)
    cost = P.costs.GaussianCost(0.3, torch.zeros(3), P.links.IdentityLinkFunction())
    dist = cost.predict(s)
    s1 = _ops.row_power_sums(s, 1)
    assert T.same_bits(host(s1), T.row_power_sums(s_host, 1)), "33 trips of the strided loop"
    assert T.same_bits(host(dist.mean), host(s1 / j))
    s2 = _ops.row_power_sums(s, 2, dist.mean)
    assert T.same_bits(host(torch.diag(dist.covariance_matrix)), host(s2 / (j - 1)))
    mean_h = host(dist.mean)
    assert max(T.row_power_sum_errors(host(s2), s_host, 2, mean_h)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# quantiles at exact ranks
def quantile_rows(rows, cols, seed):
    """magnitudes 1e-300 .. 1e300 of both signs, a quarter of each row duplicates, +-0 and subnormals; the last row seven
    distinct values (ties nearly everywhere)"""
    rng = np.random.default_rng(seed)
    x = rng.choice([-1.0, 1.0], size=(rows, cols)) * 10.0 ** rng.uniform(-300.0, 300.0, size=(rows, cols))
    for r in range(rows):
        to, frm = rng.integers(0, cols, size=cols // 4), rng.integers(0, cols, size=cols // 4)
        x[r, to] = x[r, frm]
        at = rng.choice(cols, size=9, replace=False)
        x[r, at] = [0.0, 0.0, -0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.5e-308, 5e-324]
    x[rows - 1] = rng.integers(-3, 4, size=cols) * 1e300 / 4
    assert np.isfinite(x).all()
    return x


def exact_rank_quantiles(P, rows, cols, ks, seed):
    """q = k / (cols - 1) with cols - 1 a power of two: the position q (cols - 1) is k exactly and the weight 0"""
    from projected_langevin_sampling_amd import _ops

    assert cols - 1 == 1 << int(math.log2(cols - 1))
    x = quantile_rows(rows, cols, seed)
    qs = [k / (cols - 1) for k in ks]
    assert all(q * (cols - 1) == k for q, k in zip(qs, ks))
    got = host(_ops.row_quantiles(dev(x), qs))
    want = np.sort(x, axis=1)[:, ks]
    bad = np.argwhere(~(got == want))
    assert bad.size == 0, f"{rows} x {cols}: {bad.shape[0]} quantiles are not the order statistic, first (row, k) " \
                          f"({bad[0][0]}, {ks[bad[0][1]]}): {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"


def test_quantiles_at_exact_ranks_lds_sort(P):
    exact_rank_quantiles(P, 4, 257, list(range(257)), seed=1)


@pytest.mark.parametrize("cols", [16385, 32769])
def test_quantiles_at_exact_ranks_radix_selection(P, cols):
    """nine quantiles: three launches of SEL_NQ = 4"""
    exact_rank_quantiles(P, 3, cols, [0, 1, 8191, 8192, 8193, cols - 2, cols - 1, 4097, cols - 4098], seed=cols)


# ---------------------------------------------------------------------------------------------------------------------------
# guard bands
def test_readout_entries_stay_inside_their_outputs(P):
    """each entry once at a ragged shape, ldout > width where there is one: the guards intact, every output entry written,
    the values the restated ones"""
    L = P.pkg._lib
    lib = L.load()
    st = L.stream_ptr()

    def done(out, what, rc):
        torch.cuda.synchronize()
        assert rc == OK, f"{what}: {lib.pls_last_error().decode()}"
        out.assert_intact(what)
        out.assert_written(what)

    j = 1000
    e = T.log_spread(j, seed=9)
    ed = dev(e)
    out = Guarded(8 * cdiv(j, 96), SENTINEL)
    done(out, "pls_block_means", lib.pls_block_means(ed.data_ptr(), j, 96, out.ptr, st))
    assert T.same_bits(host(out.f64()), T.block_means(e, 96))
    out = Guarded(8 * cdiv(j, 256), SENTINEL)
    done(out, "pls_chunk_sums", lib.pls_chunk_sums(ed.data_ptr(), j, out.ptr, st))
    assert T.same_bits(host(out.f64()), T.chunk_sums(e))
    out = Guarded(8 * cdiv(j, 16), SENTINEL)
    done(out, "pls_sums16", lib.pls_sums16(ed.data_ptr(), j, out.ptr, st))
    assert T.same_bits(host(out.f64()), T.sums16(e))

    rows, cols = 5, 300
    x = T.log_spread((rows, cols), seed=10)
    buf, lds = laid_out(x, 3)
    out = Guarded(8 * rows, SENTINEL)
    done(out, "pls_row_power_sums", lib.pls_row_power_sums(buf.data_ptr(), lds, rows, cols, None, 1, out.ptr, st))
    assert T.same_bits(host(out.f64()), T.row_power_sums(x, 1))

    q = torch.tensor([0.0, 0.5, 1.0, 0.25, 0.75], dtype=F64, device="cuda")
    for rows, cols, what in ((5, 301, "pls_row_quantiles, LDS sort"), (3, 16385, "pls_row_quantiles, radix selection")):
        x = T.log_spread((rows, cols), seed=cols)
        buf, lds = laid_out(x, 3)
        out = GuardedMatrix(rows, 5, 7)
        done(out, what, lib.pls_row_quantiles(buf.data_ptr(), lds, rows, cols, q.data_ptr(), 5, out.ptr, 7, st))
        srt = np.sort(x, axis=1)
        mid = [0, (cols - 1) // 2, cols - 1]  # (cols - 1 is even at both shapes: q = 0, 1/2, 1 are order statistics)
        assert np.array_equal(host(out.matrix())[:, :3], srt[:, mid]), what

    rows, cols = 1030, 300  # (more rows than the grid has: the grid-stride loop stores too)
    x = np.random.default_rng(11).standard_normal((rows, cols))
    buf, lds = laid_out(x, 3)
    out = GuardedMatrix(rows, cols, cols + 5)
    done(out, "pls_link_transform", lib.pls_link_transform(L.LINK_SQUARE, 1e-10, buf.data_ptr(), lds, rows, cols, None, out.ptr,
                                                           cols + 5, st))
    assert np.array_equal(host(out.matrix()), x * x)


# ---------------------------------------------------------------------------------------------------------------------------
# prediction, orthonormal basis
def ld(a):
    return np.asarray(a, dtype=np.longdouble)


@pytest.mark.parametrize("n,m,d,threshold,seed,n_star,j", [(600, 200, 3, 1e-8, 47, 1030, 300), (300, 12, 2, 1e-6, 31, 1, 1)])
def test_onb_prediction_per_element(P, n, m, d, threshold, seed, n_star, j):
    """Two stages, each per element against a long-double contraction (64-bit significand: its own error, K 2^-64, is inside
    the slack of 8 u).  1: pt = V~^T k(Z, x), M terms.  2: n_x + pt^T U - pt^T n_Z from the DEVICE's pt, two contractions of
    M_k terms.  1030 test points are more than rows_grid's 1024; M_k = 185 is above one 128-row tile and no multiple of 16."""
    from projected_langevin_sampling_amd import _ops

    assert np.finfo(np.longdouble).nmant >= 63, "the long-double contraction needs the x87 format"
    pr = make_problem(n, m, j, d, seed=seed)
    _, gb = build_onb(P, pr, threshold=threshold)
    mk = gb.approximation_dimension
    if m == 200:
        assert mk > 128 and mk % 16 != 0, mk
    g = pr["gen"]
    xs = torch.rand(n_star, d, generator=g) * 2 - 1
    u = torch.randn(mk, j, generator=g)
    noise = torch.randn(mk + n_star, j, generator=g)
    got = host(gb.predict_untransformed_samples(u.cuda(), xs, noise=noise.cuda()))
    assert got.shape == (n_star, j)
    v = gb.scaled_eigenvectors
    kzx = gb.kernel.base_kernel(x1=gb.x_induce, x2=xs)
    assert v.shape == (m, mk) and kzx.shape == (m, n_star)
    pt = host(_ops.gemm_tn(v, kzx))
    vh, kh, uh, nh = host(v), host(kzx), u.numpy(), noise.numpy()
    # stage 1
    want = ld(vh).T @ ld(kh)
    bound = (m + 8) * U * (ld(np.abs(vh)).T @ ld(np.abs(kh)))
    ratio = np.abs(ld(pt) - want) / bound
    print(f"V~^T k(Z,x) ({mk} x {n_star}, {m} terms): worst |error| / bound {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0, np.unravel_index(np.argmax(ratio), ratio.shape)
    # stage 2
    n_z, n_x = nh[:mk], nh[mk:]
    want = ld(n_x) + ld(pt).T @ ld(uh) - ld(pt).T @ ld(n_z)
    apt = ld(np.abs(pt)).T
    bound = (2 * mk + 8) * U * (ld(np.abs(n_x)) + apt @ ld(np.abs(uh)) + apt @ ld(np.abs(n_z)))
    ratio = np.abs(ld(got) - want) / bound
    print(f"predicted samples ({n_star} x {j}, 2 x {mk} terms): worst |error| / bound {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0, np.unravel_index(np.argmax(ratio), ratio.shape)


# ---------------------------------------------------------------------------------------------------------------------------
# link transform, tall
def native_links(P):
    Lk = P.links
    return [Lk.IdentityLinkFunction(), Lk.SquareLinkFunction(), Lk.SigmoidLinkFunction(), Lk.ProbitLinkFunction(),
            Lk.ExponentialLinkFunction()]


def test_tall_link_transform_equals_its_rows(P):
    """1030 rows on a grid of 1024: the last six come from the second trip of the loop.  Each row alone is the grid the
    per-element truths pin (tests/cost_truth.py)."""
    L = P.pkg._lib
    lib = L.load()
    rows, cols, ldin = 1030, 300, 303
    rng = np.random.default_rng(21)
    f_host = 3.0 * rng.standard_normal((rows, cols))
    f_host[rng.integers(0, rows, 64), rng.integers(0, cols, 64)] = rng.choice([-800.0, -40.0, -0.0, 0.0, 40.0, 800.0], size=64)
    eps = 0.3 * rng.standard_normal(cols)
    buf, _ = laid_out(f_host, ldin - cols)
    f = buf.as_strided((rows, cols), (ldin, 1))
    summed = dev(f_host + eps[None, :])
    kinds = set()
    for link in native_links(P):
        kinds.add(link.kind)
        name = type(link).__name__
        tall = link._native_transform(f)
        single = torch.full((rows, cols), NAN, dtype=F64, device="cuda")
        for r in range(rows):
            rc = lib.pls_link_transform(link.kind, float(link.jitter), f[r].data_ptr(), cols, 1, cols, None, single[r].data_ptr(), cols,
                                        L.stream_ptr())
            assert rc == OK, lib.pls_last_error()
        diff = (tall.view(torch.int64) != single.view(torch.int64)).nonzero()
        assert diff.numel() == 0, f"{name}: {diff.shape[0]} entries of the tall call differ from the one-row calls, first {diff[0].tolist()}"
        assert not torch.isnan(tall).any()
        cost = P.costs.GaussianCost(0.3, torch.zeros(3), link)
        got = cost.predict_samples(f, dev(eps))
        want = link._native_transform(summed)
        diff = (got.view(torch.int64) != want.view(torch.int64)).nonzero()
        assert diff.numel() == 0, f"{name}: link(f + eps) differs from the link of the host's sum at {diff[0].tolist()}"
    assert kinds == set(range(L.LINK_IDENTITY, L.LINK_EXP + 1)), "a native link is missing from this test"
