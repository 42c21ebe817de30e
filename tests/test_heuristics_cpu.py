"""CPU side of the device-evaluated env-reading heuristics (csrc/ev2g_heuristic.h): the C-ABI surface, the evaluator's dispatch, the
EV2GymVec path of the agents, and the kernel's register budget (the compiler's own figures; tests/test_heuristics_gpu.py runs them)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("ChargeAsLateAsPossible", "ChargeAsFastAsPossibleToDesiredCapacity", "RoundRobin")


def test_heuristic_kinds_mirror_the_header():
    from ev2gym_amd import _abi
    txt = open(os.path.join(ROOT, "include", "ev2g.h")).read()
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define EV2G_HEURISTIC_([A-Z_]+)\s+(\d+)", txt)}
    assert hdr == {"CHARGE_AS_LATE_AS_POSSIBLE": 0, "CHARGE_AS_FAST_TO_DESIRED_CAPACITY": 1, "ROUND_ROBIN": 2}
    assert _abi.HEURISTIC_KINDS == {"ChargeAsLateAsPossible": 0, "ChargeAsFastAsPossibleToDesiredCapacity": 1, "RoundRobin": 2}


def test_library_exports_the_heuristic_entry_points():
    from ev2gym_amd import build, engine
    L = ctypes.CDLL(build.build())
    for name in ("ev2g_heuristic_create", "ev2g_heuristic_destroy", "ev2g_heuristic_actions", "ev2g_heuristic_run"):
        assert hasattr(L, name) and name in engine.EXPORTED_SYMBOLS


class _HeuristicEngine:
    """Stand-in for ev2gym_amd.engine.Engine with the heuristic entry points (the calls evaluate() makes), recording them."""
    calls = []

    def __init__(self, batch, rk, sk):
        self.E, self.T = batch.n_envs, batch.n_steps
        self.closed = False

    def heuristic_create(self, name):
        self.calls.append(("create", name))
        return name

    def reset(self):
        self.calls.append(("reset",))

    def heuristic_run(self, a, k):
        self.calls.append(("run", a, k))
        self._last = a

    def stats(self):
        from ev2gym_amd import _abi
        return np.full((self.E, _abi.N_STATS), float(NAMES.index(self._last)))

    def check_faults(self):
        pass

    def last_step_n_kernel_ms(self):
        return 2.0

    def close(self):
        self.closed = True


def _batch():
    from ev2gym_amd.scenario_gen import GenConfig, generate
    return generate(GenConfig.v2g_profit_plus_loads(3, 6, 1, seed=4))


def test_evaluate_runs_the_env_reading_agents_through_heuristic_run():
    from ev2gym_amd.evaluator import ALGORITHMS, DEVICE_HEURISTICS, RESULT_STATS, evaluate
    assert set(DEVICE_HEURISTICS) == set(NAMES) and not set(DEVICE_HEURISTICS) & set(ALGORITHMS)
    assert evaluate.__defaults__[0] == ALGORITHMS   # the default list is unchanged
    batch = _batch()
    _HeuristicEngine.calls = []
    df = evaluate(batch, algorithms=list(NAMES), engine_factory=_HeuristicEngine)
    assert len(df) == 3 * len(NAMES) and list(df["Algorithm"].unique()) == list(NAMES)
    assert list(df.columns) == ["run", "Algorithm", "control_horizon", "discharge_price_factor"] + RESULT_STATS + ["total_reward", "time"]
    assert [c for c in _HeuristicEngine.calls if c[0] == "run"] == [("run", n, batch.n_steps) for n in NAMES]
    assert _HeuristicEngine.calls[:3] == [("create", NAMES[0]), ("reset",), ("run", NAMES[0], batch.n_steps)]
    for i, n in enumerate(NAMES):
        sub = df[df["Algorithm"] == n]
        assert sub["run"].tolist() == [0, 1, 2] and (sub["total_reward"] == float(i)).all() and (sub["time"] == 2e-3).all()


def test_evaluate_refuses_the_env_reading_agents_without_heuristic_run():
    from ev2gym_amd.evaluator import evaluate
    made = []

    class _NoHeuristics(_HeuristicEngine):
        heuristic_run = property(lambda self: (_ for _ in ()).throw(AttributeError("heuristic_run")))

        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

    for name in NAMES:
        with pytest.raises(NotImplementedError):
            evaluate(_batch(), algorithms=[name], engine_factory=_NoHeuristics)
    assert made and all(e.closed for e in made)
    with pytest.raises(NotImplementedError):
        evaluate(_batch(), algorithms=["MPC"], engine_factory=_HeuristicEngine)


class _VecStandIn:
    """What the agents see of an EV2GymVec: num_envs and the device-heuristic hooks; walking the object graph is an error."""
    num_envs = 4

    def __init__(self):
        self.created, self.asked = [], []

    @property
    def charging_stations(self):
        raise AssertionError("an EV2GymVec agent must not walk env.charging_stations")

    def heuristic_create(self, name):
        self.created.append(name)
        return ("agent", name, len(self.created))

    def heuristic_actions(self, agent):
        self.asked.append(agent)
        return "device actions"


@pytest.mark.parametrize("name", NAMES)
def test_vec_env_agents_use_the_device_and_not_the_object_graph(name):
    from ev2gym_amd.baselines import heuristics as H
    env = _VecStandIn()
    agent = getattr(H, name)(env=env)
    assert agent.get_action(env) == "device actions" and agent.get_action(env) == "device actions"
    assert env.created == [name] and env.asked == [("agent", name, 1)] * 2   # one device agent, kept across steps
    other = _VecStandIn()
    agent.get_action(other)
    assert other.created == [name]   # another env gets its own


def test_heuristic_kernel_compiles_without_spills_or_scratch(tmp_path):
    """Every instantiation of ev2g_heuristic_kernel stays well inside the register file without scratch (the compiler's own figures,
    -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
    from ev2gym_amd import build
    src = tmp_path / "heur.hip"
    src.write_text('#include "ev2g_heuristic.h"\n'
                   "template __global__ void ev2g_heuristic_kernel<0>(DevScn, DevState, HeurArgs, int, double *);\n"
                   "template __global__ void ev2g_heuristic_kernel<1>(DevScn, DevState, HeurArgs, int, double *);\n"
                   "template __global__ void ev2g_heuristic_kernel<2>(DevScn, DevState, HeurArgs, int, double *);\n")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-I", os.path.join(ROOT, "ev2gym_amd", "csrc"), "--cuda-device-only", "-c",
                                     "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, str(src)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur:
            res.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    heur = {k: v for k, v in res.items() if "ev2g_heuristic_kernel" in k}
    assert len(heur) == 3, sorted(res)
    for k, v in heur.items():
        assert v["VGPRs"] <= 64 and v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
