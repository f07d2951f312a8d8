"""Writes tests/golden/<family>_cost_reference_errors.json for a family of tests/cost_families.py (count, beta, ordinal, gamma): the
largest error of the family's host restatement (fp64 torch; tests/<family>_cost_truth.py) against the mpmath truth, per (pair, parameter set,
value / derivative mode / link, regime) -- for beta also of torch's lgamma / digamma / x digamma per regime of the special
functions' points -- in the regime's unit.  Recorded results only; tests/test_<family>_cost_host.py re-checks the file against
a fresh run.

    python tests/golden/make_cost_reference_errors.py count|beta|ordinal|gamma"""
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
    import cost_families

    (family,) = sys.argv[1:]
    (module,) = [m for m in cost_families.FAMILIES if cost_families.family_name(m) == family]
    measured = module.measure_reference()
    with open(os.path.join(HERE, f"{family}_cost_reference_errors.json"), "w") as fh:
        json.dump(encode(measured), fh, indent=1, sort_keys=True)
        fh.write("\n")
