"""The loader's host-only plan (csrc/ev2g_load_host.h) on a machine without a GPU: tests/host/load_plan_check.cpp builds its batches in
code and checks the session order, the first-free port replay, the chained windows, the dictionary and every refusal of the plan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_load_plan_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "load_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "load_plan_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "load_plan_check: ok" in run.stdout
