"""The learners' host-only description (csrc/ev2g_learner_host.h: LearnerSpec, learner_spec, learner_refusal, adam_step, rms_step,
learner_host_head) on a machine without a GPU: tests/host/learner_check.cpp checks that SB3's default PPO and A2C configs (RMSprop and Adam)
resolve to the head, optimiser, constants and hyper-parameters written out by hand, that every out-of-range, NaN and infinite value of every
config field is refused with the ABI's literal message and the earlier of two bad fields is the one named, and that the optimiser step structs
equal independently written expressions."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_learner_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "learner_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "learner_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "learner_check: ok" in run.stdout
