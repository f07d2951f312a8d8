"""GPU: the orthonormal basis built FROM DATA in plain C++ (examples/cabi_onb_from_data.cpp) -- points -> pls_kernel_gram ->
pls_sym_eigh -> threshold and scale -> pls_onb_build_projection -> one pls_onb_step, no torch and no Python on the data
path.  The program checks itself against a scalar restatement; here it is compiled and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_onb_from_data_in_plain_cpp(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    libdir = os.path.join(ROOT, "projected-langevin-sampling_amd")
    assert os.path.exists(os.path.join(libdir, "libplship.so")), "build the library first (__graft_entry__.build())"
    exe = str(tmp_path / "cabi_onb_from_data")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "cabi_onb_from_data.cpp"), "-L", libdir, "-lplship", f"-Wl,-rpath,{libdir}",
                    "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cabi_onb_from_data OK" in run.stdout and "eigh: info 0" in run.stdout
