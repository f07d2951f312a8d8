"""GPU: the element-wise entries -- pls_cost_derivative (both derivative modes), pls_cost_value and pls_link_transform,
through calculate_cost_derivative / calculate_cost / the link's transform -- against the per-element mpmath truth of
tests/cost_truth.py on its whole grid: bulk, both tails out to overflow, both sides of each clip bound, the Poisson pole and
root, the multimodal tie, +-0 and subnormals, with every row its own y and mixed labels, N and J off every multiple of 4.

The bound is not fixed in advance: per (pair, parameter set, kind, regime) the GPU's largest error, in the regime's unit, may
be 4x the oracle's recorded one (tests/golden/cost_truth_oracle_errors.json) or 4 units, whichever is larger
(cost_truth.bound).  IEEE specials must match exactly.  PLS_COST_TRUTH_DUMP=<file> appends the measured maxima as JSON lines
(the table of DESIGN.md section 3 is made from them)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import cost_truth as T
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _dump(record):
    path = os.environ.get("PLS_COST_TRUTH_DUMP")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(record) + "\n")


def gpu_eval(P, T, pair, pset, kind, strided=False):
    """the library on the grid of the truth module ``T``, per element (N, J); ``strided``: the samples are the left columns of
    a wider matrix"""
    y, f, _ = T.grid(pair, pset)
    yt, ft = torch.as_tensor(y), torch.as_tensor(f).cuda()
    if strided:
        wide = torch.full((f.shape[0], f.shape[1] + 3), float("nan"), device="cuda")
        wide[:, :f.shape[1]] = ft
        ft = wide[:, :f.shape[1]]
    if kind == "link":
        return T.gpu_cost(P, pair, pset, yt).link_function(ft).cpu().numpy()
    if kind == "value":  # the entry sums over rows: one row at a time
        rows = [T.gpu_cost(P, pair, pset, yt[a:a + 1]).calculate_cost(ft[a:a + 1]) for a in range(len(y))]
        return torch.stack(rows).cpu().numpy()
    return T.gpu_cost(P, pair, pset, yt).calculate_cost_derivative(ft, force_autograd=kind == "deriv_autograd").cpu().numpy()


def elements_against_truth(P, T, pair, pset, reference="host"):
    """Every kind the pair has, dense and strided, per regime within the bound its recorded reference error sets
    (``reference``: what the printed line calls it).  Returns {(kind, strided): the library's (N, J) values}, for the asserts
    a family adds of its own."""
    rec = T.reference_errors()[pair][pset]
    regimes = T.grid(pair, pset)[2]
    got, missed = {}, []
    for kind in T.KINDS:
        if not T.applies(pair, kind):
            continue
        tr = T.truth(pair, pset, kind)
        for strided in (False, True):
            got[kind, strided] = gpu_eval(P, T, pair, pset, kind, strided)
            err = T.by_regime(T.errors(got[kind, strided], tr), regimes)
            for regime, v in err.items():
                bound = T.bound(rec[kind][regime])
                print(f"{pair} {pset} {kind:16s} {regime:10s} gpu {v:10.3g}  {reference} {rec[kind][regime]!s:>10}  bound {bound:.3g}")
                if not strided:
                    _dump({"pair": pair, "pset": pset, "kind": kind, "regime": regime, "gpu": v if math.isfinite(v) else "inf",
                           "oracle": rec[kind][regime]})
                if not v <= bound:
                    missed.append((kind, regime, "strided" if strided else "dense", v, bound))
    assert not missed, f"{pair} {pset}: cells over their bound (kind, regime, layout, error, bound): {missed}"
    return got


def modes_agree(got):
    """for a family whose two derivative modes are one formula: the same bits, dense and strided"""
    for strided in (False, True):
        assert np.array_equal(got["deriv_reference", strided], got["deriv_autograd", strided], equal_nan=True), "the two derivative modes differ"


def value_column_sums(P, T, pair, pset):
    """calculate_cost on the whole matrix (every row slot of the kernel, mixed labels within a register's rows): the sum
    over rows against the truth's, at the cells' bounds of elements_against_truth plus the N roundings of the sum"""
    y, f, regimes = T.grid(pair, pset)
    rec = T.reference_errors()[pair][pset]["value"]
    tr = T.truth(pair, pset, "value")
    got = T.gpu_cost(P, pair, pset, torch.as_tensor(y)).calculate_cost(torch.as_tensor(f).cuda()).cpu().numpy()
    n = len(y)
    for b, regime in enumerate(regimes):
        hi = tr["hi"][:, b]
        if not np.isfinite(hi).all():  # IEEE specials: what the sum of the truths gives
            with np.errstate(invalid="ignore"):
                want = hi.sum()
            assert (np.isnan(want) and np.isnan(got[b])) or got[b] == want, (pair, pset, regime, b, got[b], want)
            continue
        want = math.fsum(hi) + math.fsum(tr["lo"][:, b])
        tol = T.bound(rec[regime]) * float(tr["unit"][:, b].sum()) + n * 2.0 ** -53 * float(np.abs(hi).sum())
        assert abs(got[b] - want) <= tol, (pair, pset, regime, b, got[b], want, abs(got[b] - want) / tol)


@pytest.mark.parametrize("pair,pset", T.cells())
def test_elements_against_truth(P, pair, pset):
    elements_against_truth(P, T, pair, pset, reference="oracle")


@pytest.mark.parametrize("pair,pset", T.cells())
def test_value_column_sums(P, pair, pset):
    value_column_sums(P, T, pair, pset)
