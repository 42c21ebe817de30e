"""The TRPO learner's host-only half (csrc/ev2g_trpo_host.h: plan_trpo, trpo_map, the config's field table, the host twins of the
conjugate-gradient iteration and of the line search's row terms) on a machine without a GPU: tests/host/trpo_check.cpp, a plain C++17 program,
checks the plan against PPO's (accepted networks, refusals, LDS never larger, blocks that tile the allocation), the flat actor order and map,
every config refusal by name, and the twins against expressions written independently there."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trpo_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "trpo_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "trpo_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "trpo_check: ok" in run.stdout
