"""What the truth modules (exact_gp_truth, dirichlet_gp_truth, svgp_truth) share: seeded inputs from integer draws, their
SHA-256, the fixtures under tests/golden/ with the guard on that checksum, and the error against a (hi, lo) truth.

The fixtures hold results, not inputs, so every machine must regenerate the inputs to the bit.  torch.randn, torch.sin and
BLAS take different code paths on different CPUs: integer draws and correctly rounded elementwise operations only, sums in a
fixed order."""
import hashlib

import numpy as np
import torch


def _uniform(g, shape):
    """uniform on [0, 1) from 30-bit integer draws: the same doubles on every machine"""
    return torch.randint(0, 2**30, shape, generator=g, dtype=torch.int64).double() / 2.0**30


def _normal(g, shape):
    """N(0, 1) as the sum of twelve uniforms minus 6 (mean 0, variance 1, exact additions)"""
    total = torch.zeros(shape, dtype=torch.float64)
    for _ in range(12):
        total = total + _uniform(g, shape)
    return total - 6.0


def checksum(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


_files = {}


def fixture_truth(path, name, inputs):
    """the 50-digit outputs of case ``name`` in the fixture at ``path`` as (hi, lo) float64 pairs, after checking that the
    regenerated ``inputs`` (a list of tensors) are the recorded ones"""
    if path not in _files:
        with np.load(path) as f:
            _files[path] = {k: f[k] for k in f.files}
    file = _files[path]
    assert str(file[f"{name}/sha256"]) == checksum(inputs), f"{name}: the regenerated inputs are not the fixture's"
    return file[f"{name}/hi"], file[f"{name}/lo"]


def relative_error(got, hi, lo, scale):
    """|got - truth| / scale per output; where the scale is 0 (every term is 0) only the exact value passes"""
    err = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
