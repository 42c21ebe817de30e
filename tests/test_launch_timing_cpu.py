"""The ring of timed calls and the stamp arithmetic (csrc/ev2g_timing_host.h) on a machine without a GPU: tests/host/timing_check.cpp holds the slot
of every `back` over several wraps, what error exits leave behind, the kind of each slot and the conversion from clock ticks to milliseconds;
tests/host/stamp_rule_check.cpp holds the host's choice of stamped launches to the rule the kernel is compiled under -- each
once plain, once as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
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
def test_timing_check(flags, tmp_path):
    exe = str(tmp_path / "timing_check")
    subprocess.check_call([_cxx(), "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "host", "timing_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "timing_check: ok" in run.stdout


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_stamp_rule_check(flags, tmp_path):
    """route_step's StepRoute::stamps against the rule the kernel compiles its stamp sites under (tests/host/stamp_rule_check.cpp)."""
    exe = str(tmp_path / "stamp_rule_check")
    subprocess.check_call([_cxx(), "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "host", "stamp_rule_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stamp_rule_check: ok" in run.stdout
