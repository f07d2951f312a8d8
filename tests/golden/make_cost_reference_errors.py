"""Writes tests/golden/<family>_cost_reference_errors.json for the family count, beta or ordinal: the largest error of the
family's host restatement (fp64 torch; tests/<family>_cost_truth.py) against the mpmath truth, per (pair, parameter set,
value / derivative mode / link, regime) -- for beta also of torch's lgamma / digamma / x digamma per regime of the special
functions' points -- in the regime's unit.  Recorded results only; tests/test_<family>_cost_host.py re-checks the file against
a fresh run.

    python tests/golden/make_cost_reference_errors.py count|beta|ordinal"""
import importlib
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]


def encode(v):
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items()}
    return "inf" if math.isinf(v) else float(f"{v:.4g}")


if __name__ == "__main__":
    (family,) = sys.argv[1:]
    assert family in ("count", "beta", "ordinal"), family
    measured = importlib.import_module(f"{family}_cost_truth").measure_reference()
    with open(os.path.join(HERE, f"{family}_cost_reference_errors.json"), "w") as fh:
        json.dump(encode(measured), fh, indent=1, sort_keys=True)
        fh.write("\n")
