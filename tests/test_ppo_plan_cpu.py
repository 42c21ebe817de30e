"""The PPO learner's host-only plan and the index its device repack writes by (csrc/ev2g_policy_host.h: plan_ppo, ppo_lds, packed_f32_index,
unpack_linear_f32) on a machine without a GPU: tests/host/ppo_plan_check.cpp checks that writing the real elements by packed_f32_index into a
zeroed image reproduces pack_linear_f32's image (so what the repack never writes is exactly the padding), that the unpack inverts the pack,
that every network the contract names is accepted with non-overlapping LDS blocks within 160 KiB and non-overlapping slab regions, and that a
refusal names the width.  The networks tests/test_learner_shapes_gpu.py runs on the device (tests/learner_cases.py: LEARNER_NETS) are pinned here
too: each is accepted with exactly the LDS bytes its row lists, so a change to the LDS plan that moves or refuses one fails without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ppo_plan_check(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "ppo_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "ppo_plan_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ppo_plan_check: ok" in run.stdout


def test_the_learner_shape_table_is_accepted_with_its_lds_bytes():
    from ev2gym_amd.engine import ppo_query
    from tests.learner_cases import LEARNER_NETS, NEAREST_THE_LDS_LIMIT, net_shape
    txt = open(os.path.join(ROOT, "ev2gym_amd", "csrc", "ev2g_policy_host.h")).read()
    a, b = re.search(r"#define EV2G_PPO_LDS_LIMIT \((\d+) \* (\d+)\)", txt).groups()
    limit = int(a) * int(b)
    lds = {}
    for tag, (d_in, h, v, d_out, activations, lds_bytes) in LEARNER_NETS.items():
        info = ppo_query(*net_shape(tag))   # (a refusal raises EngineError with the plan's message)
        lds[tag] = info["lds_bytes"]
        assert info["lds_bytes"] == lds_bytes, (tag, info)
        assert info["lds_bytes"] <= limit and info["grid_cap"] >= 1 and activations
    assert max(lds, key=lds.get) == NEAREST_THE_LDS_LIMIT and limit - lds[NEAREST_THE_LDS_LIMIT] == 1664, lds
