"""A step launch's route (csrc/ev2g_route_host.h) on a machine without a GPU: tests/host/route_check.cpp enumerates the loaded shapes and the
calls and checks the instantiation, the reported specialisation, the fast-forward and in-launch statistics flags, both reason ladders, the
collectors' direct route and the fused launch's table index against predicates restated from the contract."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "route_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "route_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "route_check: ok" in run.stdout
