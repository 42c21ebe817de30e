"""The CU-balance maps (csrc/ev2g_balance_host.h) on a machine without a GPU: tests/host/balance_check.cpp holds the live-step weights, the order in
which workgroups take groups and the map itself against brute force -- once plain, once as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    return cxx


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_balance_check(flags, tmp_path):
    exe = str(tmp_path / "balance_check")
    subprocess.check_call([_cxx(), "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "host", "balance_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "balance_check: ok" in run.stdout
