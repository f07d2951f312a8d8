"""CPU: the host side of the symmetric eigensolver (pls_sym_eigh, csrc/sym_eigh.hip) -- argument validation through the
built library (it happens before any HIP call), the workspace formula, the round-robin schedule, the Python routing of
eigh_device="plship", and the committed truth (tests/golden/sym_eigh_truth.npz) against LAPACK."""
import ctypes as C

import numpy as np
import pytest
import torch

import sym_eigh_truth as T


@pytest.fixture(scope="module")
def lib():
    import projected_langevin_sampling_amd as pkg

    return pkg._lib.load()


def _call(lib, a, lda, m, lam, v, ldv, info, ws, ws_bytes):
    return lib.pls_sym_eigh(a, lda, m, lam, v, ldv, info, ws, ws_bytes, None)


def test_arguments_are_validated_before_any_hip_call(lib):
    buf = (C.c_double * 64)()
    p = C.addressof(buf)  # a non-NULL address; no valid call below reaches the device
    info = C.c_int32(7)
    need = lib.pls_sym_eigh_workspace_bytes(5)
    bad = [
        (dict(a=None), b"NULL"), (dict(lam=None), b"NULL"), (dict(v=None), b"NULL"), (dict(info=None), b"NULL"),
        (dict(ws=None), b"NULL"), (dict(lda=4), b"lda"), (dict(ldv=4), b"ldv"), (dict(m=-1), b"m = -1"),
        (dict(ws_bytes=need - 8), b"workspace"),
    ]
    for change, text in bad:
        kw = dict(a=p, lda=5, m=5, lam=p, v=p, ldv=5, info=C.byref(info), ws=p, ws_bytes=need)
        kw.update(change)
        rc = _call(lib, kw["a"], kw["lda"], kw["m"], kw["lam"], kw["v"], kw["ldv"], kw["info"], kw["ws"], kw["ws_bytes"])
        assert rc == 1, change
        assert text in lib.pls_last_error(), (change, lib.pls_last_error())
    assert info.value == 7  # untouched


def test_order_zero_succeeds_and_touches_nothing(lib):
    info = C.c_int32(7)
    assert _call(lib, None, 0, 0, None, None, 0, C.byref(info), None, 0) == 0
    assert info.value == 7
    assert lib.pls_sym_eigh_workspace_bytes(0) == 0


def test_workspace_formula(lib):
    sizes = [lib.pls_sym_eigh_workspace_bytes(m) for m in range(0, 1100)]
    assert all(s % 8 == 0 for s in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] > 0
    # two m x m planes (the working matrix and the rotations) at the padded order are the bulk of it
    assert sizes[1024] >= 2 * 1024 * 1024 * 8


@pytest.mark.parametrize("nblocks", range(2, 18))
def test_round_robin_schedule(lib, nblocks):
    rounds = nblocks - 1 if nblocks % 2 == 0 else nblocks
    seen = set()
    for r in range(rounds):
        pairs = (C.c_int64 * (2 * (nblocks // 2)))()
        count = lib.pls_sym_eigh_round_pairs(nblocks, r, pairs)
        assert count == nblocks // 2  # (an odd count: one block has a bye)
        got = [(pairs[2 * k], pairs[2 * k + 1]) for k in range(count)]
        flat = [b for pr in got for b in pr]
        assert len(set(flat)) == len(flat), "pairs of a round are disjoint"
        assert all(0 <= i < j < nblocks for i, j in got)
        if nblocks % 2:
            assert len(set(range(nblocks)) - set(flat)) == 1
        for pr in got:
            assert pr not in seen, "a pair occurs once per sweep"
            seen.add(pr)
    assert len(seen) == nblocks * (nblocks - 1) // 2
    pairs = (C.c_int64 * 64)()
    assert lib.pls_sym_eigh_round_pairs(nblocks, rounds, pairs) == 0 and lib.pls_sym_eigh_round_pairs(nblocks, -1, pairs) == 0


def test_resolve_eigh_device_accepts_plship_and_auto_never_gives_it():
    from projected_langevin_sampling_amd import samplers

    small, large = torch.zeros(4, 4), torch.zeros(300, 300)
    assert samplers.resolve_eigh_device("plship", small) == "plship"
    assert samplers.resolve_eigh_device("plship", large) == "plship"
    prev = samplers.DEFAULT_EIGH_DEVICE
    try:
        samplers.DEFAULT_EIGH_DEVICE = "plship"
        assert samplers.resolve_eigh_device(None, large) == "plship"
        samplers.DEFAULT_EIGH_DEVICE = "auto"
        for mat in (small, large, torch.zeros(300, 300, device="meta")):
            assert samplers.resolve_eigh_device(None, mat) in ("cpu", "cuda")
            assert samplers.resolve_eigh_device("auto", mat) in ("cpu", "cuda")
    finally:
        samplers.DEFAULT_EIGH_DEVICE = prev
    assert samplers.EIGH_HOST_BELOW == 128
    with pytest.raises(AssertionError):
        samplers.resolve_eigh_device("rocsolver", small)


def test_canonicalise_signs_is_idempotent():
    from projected_langevin_sampling_amd.basis.spectrum import canonicalise_signs

    g = torch.Generator().manual_seed(5)
    v = torch.randn(9, 9, generator=g, dtype=torch.float64)
    v[:, 3] = torch.tensor([0.5, -0.5, 0.1, 0, 0, 0, 0, 0, 0.5])  # a tie: the first maximal component decides
    v[:, 4] = 0.0
    once = canonicalise_signs(v)
    assert torch.equal(canonicalise_signs(once), once)
    assert torch.equal(once.abs(), v.abs())
    pivot = once.abs().argmax(dim=0)
    assert bool((once.gather(0, pivot[None, :]) >= 0).all()) and once[0, 3] == 0.5


def test_truth_file_agrees_with_lapack():
    """mpmath's 50-digit eigenvalues against numpy.linalg.eigvalsh.  LAPACK is backward stable: its eigenvalues are those of
    A + E with ||E||_2 <= p(M) eps ||A||_2 for a modest p; the cap is the 4 M eps ||A||_2 the solver is held to
    (measured: below 4 eps ||A||_2 on the rbf cases)."""
    truth = T.load_truth()
    assert set(truth) == {(f, m) for f in T.FAMILIES for m in T.FIXTURE_SIZES}
    for (family, m), (a, lam) in truth.items():
        assert a.shape == (m, m) and np.array_equal(a, a.T) and np.all(np.diff(lam) >= 0)
        assert np.array_equal(a, T.make_matrix(family, m)) or np.allclose(a, T.make_matrix(family, m), rtol=1e-13, atol=0)
        scale = np.abs(lam).max()
        err = np.abs(np.linalg.eigvalsh(a) - lam).max()
        assert err <= 4 * m * T.EPS * scale, (family, m, err / (T.EPS * scale))
    assert np.all(np.diff(truth[("indef", 130)][1]) > 0) and truth[("indef", 130)][1][0] < 0 < truth[("indef", 130)][1][-1]
    lam = truth[("doubled", 96)][1]
    assert np.array_equal(lam[0::2], lam[1::2])
