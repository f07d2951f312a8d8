"""GPU: bench.py's plain run prints the headline and nothing the headline does not need; `--dump-outputs` writes the
particles of the last timed step, and two runs with the same arguments agree on them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(*args):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_plain_bench_line_is_the_headline_and_its_dump_repeats(tmp_path):
    lines = [_bench_line("--gpus", "1", "--config", "small", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
             for d in ("a", "b")]
    extras = {"roofline", "roofline_gram", "sustained", "gaussian_fast_path", "converged_energy", "train_pls_iteration",
              "inducing_point_basis", "shard_check", "construct_plus_T_steps", "reference_scale", "cpu_baseline", "gpu_over_cpu"}
    for line in lines:
        assert line["metric"] == "Langevin steps/sec" and line["unit"] == "steps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-9 * 1e3
        assert not extras & set(line), sorted(extras & set(line))
    a, b = (np.load(tmp_path / d / "particles.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (lines[0]["config"]["M_k"], lines[0]["config"]["J"])
    assert np.isfinite(a).all()
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-12 * np.abs(a).max())
