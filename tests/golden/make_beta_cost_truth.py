"""Writes tests/golden/beta_cost_reference_errors.json: the largest error of the host restatement of the Beta cost (fp64 torch;
tests/beta_cost_truth.py) against the mpmath truth, per (pair, parameter set, value / derivative mode, regime), and of torch's
lgamma / digamma / x digamma per regime of the special functions' points, in the regime's unit.  Recorded results only;
tests/test_beta_cost_host.py re-checks the file against a fresh run.

    python tests/golden/make_beta_cost_truth.py"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import beta_cost_truth  # noqa: E402


def encode(v):
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items()}
    return "inf" if math.isinf(v) else float(f"{v:.4g}")


if __name__ == "__main__":
    with open(os.path.join(HERE, "beta_cost_reference_errors.json"), "w") as fh:
        json.dump(encode(beta_cost_truth.measure_reference()), fh, indent=1, sort_keys=True)
        fh.write("\n")
