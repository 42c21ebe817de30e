"""The pinning recipe itself is under test: the scripts that hold oracle/ev2g_oracle.c to the LIVE
reference must start at HEAD.  Those tests need a checkout of the upstream reference at oracle.ref_import.REF_ROOT and skip where
there is none (it is not part of this repository; the committed fixtures under tests/golden/ carry its results everywhere else).
Each script runs in its own process: they chdir into the reference tree and install import stubs."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REF_ROOT  # noqa: E402

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF_ROOT, "ev2gym")),
                                     reason=f"no checkout of the upstream reference at {REF_ROOT} (not part of this repository)")


def _run(args, env=None, timeout=900):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=tempfile.gettempdir(), timeout=timeout,
                       env={**os.environ, **(env or {})})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


@needs_reference
def test_differential_fuzz_against_the_live_reference_starts_and_agrees():
    out = _run([os.path.join(ROOT, "oracle", "fuzz_vs_reference.py"), "2"])
    last = out.strip().splitlines()[-1]
    assert last.startswith("2 cases"), out[-500:]
    assert float(last.split()[-1]) < 1e-12


@needs_reference
def test_capture_script_regenerates_committed_fixtures(tmp_path):
    """One `agent_*` and one `b2b_*` case: the two families that import ev2gym_amd after the reference (the ones that broke); two `edge_*`
    cases: their actions come from tests/threshold_cases.py, one of them through the scenario the reference drew (the `gate` policy)."""
    names = ["agent_roundrobin_pst_s61", "b2b_pst_rand_s53", "edge_topo_v2gppl_het_gate_s98", "edge_v2gppl_p2_latwild_s95"]
    _run([os.path.join(ROOT, "oracle", "capture_golden.py")] + names, env={"EV2G_GOLDEN_OUT": str(tmp_path)})
    for n in names:
        new, old = np.load(tmp_path / (n + ".npz"), allow_pickle=False), np.load(os.path.join(ROOT, "tests", "golden", n + ".npz"), allow_pickle=False)
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k], equal_nan=old[k].dtype.kind == "f"), (n, k)   # NaN marks empty ports in the trajectories


@needs_reference
def test_live_reference_checks_of_back_to_back_sessions_and_written_replays_start():
    assert _run([os.path.join(ROOT, "oracle", "check_back_to_back.py")]).strip().endswith("OK")
    assert _run([os.path.join(ROOT, "oracle", "check_replay_write.py")]).strip().endswith("OK")


def test_a_partial_gymnasium_in_sys_modules_never_breaks_the_import():
    code = ("import sys, types; g = types.ModuleType('gymnasium'); sys.modules['gymnasium'] = g; "
            f"sys.path.insert(0, {ROOT!r}); import ev2gym_amd; from ev2gym_amd import gym_compat; "
            "assert gym_compat.register_gym_id() is False; print('ok')")
    assert _run(["-c", code]).strip() == "ok"
