"""Writes tests/golden/gamma_cost_reference_errors.json: the largest error of the Gamma cost's host restatement (fp64 torch;
tests/gamma_cost_truth.py) against the mpmath truth, per (pair, parameter set, value / derivative mode, regime), in the regime's
unit.  Recorded results only; tests/test_gamma_cost_host.py re-checks the file against a fresh run.

    python tests/golden/make_gamma_cost_truth.py"""
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
    import gamma_cost_truth

    with open(os.path.join(HERE, "gamma_cost_reference_errors.json"), "w") as fh:
        json.dump(encode(gamma_cost_truth.measure_reference()), fh, indent=1, sort_keys=True)
        fh.write("\n")
