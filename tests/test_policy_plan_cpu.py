"""A policy's plan and weight images (csrc/ev2g_policy_host.h) on a machine without a GPU: tests/host/policy_plan_check.cpp enumerates the
network shapes and precisions and checks the chosen actor kernel, its fragment packing, LDS bytes, rows and threads, the refusals and the
table's index functions against predicates restated from the contract; then every element of the three weight layouts, the bias images and
the actor-critic's twelve arrays against the index each layout documents, and the bf16 rounding against one written on the word's halves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_plan_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "policy_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "policy_plan_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "policy_plan_check: ok" in run.stdout
