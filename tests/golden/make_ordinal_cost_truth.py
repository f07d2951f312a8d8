"""Writes tests/golden/ordinal_cost_reference_errors.json: the largest error of the host restatement of the ordinal cost (fp64
torch; tests/ordinal_cost_truth.py) against the mpmath truth, per (pair, parameter set, value / derivative mode, regime),
in the regime's unit.  Recorded results only; tests/test_ordinal_cost_host.py re-checks the file against a fresh run.

    python tests/golden/make_ordinal_cost_truth.py"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import ordinal_cost_truth  # noqa: E402


def encode(v):
    return "inf" if math.isinf(v) else float(f"{v:.4g}")


if __name__ == "__main__":
    m = ordinal_cost_truth.measure_reference()
    out = {p: {s: {k: {r: encode(v) for r, v in c.items()} for k, c in ks.items()} for s, ks in ss.items()} for p, ss in m.items()}
    with open(os.path.join(HERE, "ordinal_cost_reference_errors.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
