"""CPU: csrc/gemm_plan.h -- the host code that decides what every GEMM launches -- compiled on its own with the system C++ compiler
under AddressSanitizer + UBSan and swept by tests/host/gemm_plan_sweep.cpp (a stand-alone program, run as a child process): the
grouped-wgrad tile ordering and split choice over the GPU tests' job lists, the MAE step's and a few hundred random ones, and
plan_gemm's workspace request against the plan it makes for a workspace of that size, over a grid of shapes, CU counts and tunings."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) if c else None
        if path:
            return path
    return None


def test_gemm_plan_sweep_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "gemm_plan_sweep")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host", "gemm_plan_sweep.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].startswith("ok "), run.stdout
