"""Writes tests/golden/cost_truth_oracle_errors.json: the oracle's (fp64 torch on the host) largest error against the mpmath
truth of tests/cost_truth.py, per (pair, parameter set, value / derivative mode / link, regime), in the regime's unit (ulps
of the truth, or 2^-53 x the cancelling terms; see tests/cost_truth.py).  Recorded results only; "inf" marks a cell where
the oracle returns a special the truth does not (its autograd's NaN where the sigmoid's exp overflows).
tests/test_cost_truth_host.py re-checks the file against a fresh run.

    python tests/golden/make_cost_truth_oracle_errors.py"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import cost_truth  # noqa: E402


def encode(v):
    return "inf" if math.isinf(v) else float(f"{v:.4g}")


if __name__ == "__main__":
    m = cost_truth.measure_oracle()
    out = {p: {s: {k: {r: encode(v) for r, v in c.items()} for k, c in ks.items()} for s, ks in ss.items()} for p, ss in m.items()}
    with open(os.path.join(HERE, "cost_truth_oracle_errors.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
