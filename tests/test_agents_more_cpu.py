"""CPU side of the three later device agents (ChargeAsLateAsPossibleToDesiredCapacity, RoundRobin_GF, RoundRobin_GF_off_allowed; kinds 3-5 of
csrc/ev2g_heuristic.h): the kind table against the header, the evaluator's dispatch, the EV2GymVec path of the facade agents, the facade
agents against the reference's own (where a checkout of it exists) and the new instantiations' register budget."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ChargeAsLateAsPossibleToDesiredCapacity", "RoundRobin_GF", "RoundRobin_GF_off_allowed")


def test_agent_kinds_mirror_the_header():
    from ev2gym_amd import _abi
    txt = open(os.path.join(ROOT, "include", "ev2g.h")).read()
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define EV2G_(?:HEURISTIC|AGENT)_([A-Z_]+)\s+(\d+)", txt)}
    assert hdr == {"CHARGE_AS_LATE_AS_POSSIBLE": 0, "CHARGE_AS_FAST_TO_DESIRED_CAPACITY": 1, "ROUND_ROBIN": 2,
                   "CHARGE_AS_LATE_TO_DESIRED_CAPACITY": 3, "ROUND_ROBIN_GF": 4, "ROUND_ROBIN_GF_OFF_ALLOWED": 5}
    new = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define EV2G_AGENT_([A-Z_]+)\s+(\d+)", txt)}
    assert sorted(new.values()) == [3, 4, 5]
    assert _abi.AGENT_KINDS == {"ChargeAsLateAsPossible": 0, "ChargeAsFastAsPossibleToDesiredCapacity": 1, "RoundRobin": 2,
                                "ChargeAsLateAsPossibleToDesiredCapacity": 3, "RoundRobin_GF": 4, "RoundRobin_GF_off_allowed": 5}
    assert list(_abi.AGENT_KINDS.items())[:3] == list(_abi.HEURISTIC_KINDS.items())
    assert tuple(_abi.AGENT_KINDS)[3:] == NEW
    assert re.search(r"#define EV2G_ABI_VERSION\s+4\b", txt)   # additive: the ABI version stays


class _Engine:
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
        return np.full((self.E, _abi.N_STATS), float(_abi.AGENT_KINDS[self._last]))

    def check_faults(self):
        pass

    def last_step_n_kernel_ms(self):
        return 2.0

    def close(self):
        self.closed = True


def _batch():
    from ev2gym_amd.scenario_gen import GenConfig, generate
    return generate(GenConfig.v2g_profit_plus_loads(3, 6, 1, seed=4))


def test_evaluate_runs_the_new_agents_through_heuristic_run_and_refuses_unknown_names():
    from ev2gym_amd import _abi
    from ev2gym_amd.evaluator import ALGORITHMS, DEVICE_AGENTS, DEVICE_HEURISTICS, evaluate
    assert DEVICE_AGENTS == tuple(_abi.AGENT_KINDS) and DEVICE_AGENTS[:3] == DEVICE_HEURISTICS and DEVICE_AGENTS[3:] == NEW
    assert not set(DEVICE_AGENTS) & set(ALGORITHMS) and evaluate.__defaults__[0] == ALGORITHMS
    batch = _batch()
    _Engine.calls = []
    df = evaluate(batch, algorithms=list(NEW), engine_factory=_Engine)
    assert len(df) == 3 * len(NEW) and list(df["Algorithm"].unique()) == list(NEW)
    assert _Engine.calls == [c for n in NEW for c in (("create", n), ("reset",), ("run", n, batch.n_steps))]
    for n in NEW:
        sub = df[df["Algorithm"] == n]
        assert sub["run"].tolist() == [0, 1, 2] and (sub["total_reward"] == float(_abi.AGENT_KINDS[n])).all()
    for name in ("ChargeAsFastAsPossibleWithPowerLimit", "MPC", "RoundRobin_GF "):
        with pytest.raises(NotImplementedError) as ei:
            evaluate(batch, algorithms=[name], engine_factory=_Engine)
        assert "RoundRobin_GF_off_allowed" in str(ei.value)   # the message lists what the device evaluates


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


@pytest.mark.parametrize("name", NEW)
def test_vec_env_agents_use_the_device_and_not_the_object_graph(name):
    from ev2gym_amd.baselines import heuristics as H
    env = _VecStandIn()
    agent = getattr(H, name)(env=env)
    assert agent.get_action(env) == "device actions" and agent.get_action(env) == "device actions"
    assert env.created == [name] and env.asked == [("agent", name, 1)] * 2


_LOCKSTEP = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(1, sys.argv[1])
import capture_golden as cg
cg.import_reference()
from ev2gym.models.ev2gym_env import EV2Gym
import ev2gym.rl_agent.state as S
import ev2gym.rl_agent.reward as RW
import ev2gym.baselines.heuristics as H
import ev2gym_amd.baselines.heuristics as MINE
base = "ev2gym/example_config_files/"
short = {"simulation_length": 60, "spawn_multiplier": 10}
des80 = cg._yaml_variant(base + "V2GProfitPlusLoads.yaml", {**short, "ev": {"desired_capacity": 0.8}}, "lockstep_des80")
pst = cg._yaml_variant(base + "PublicPST.yaml", short, "lockstep_pst")
PPL, PST = ("V2G_profit_max_loads", "ProfitMax_TrPenalty_UserIncentives"), ("PublicPST", "SquaredTrackingErrorReward")
for name, cfg, (sf, rf) in (("ChargeAsLateAsPossibleToDesiredCapacity", des80, PPL), ("RoundRobin_GF", pst, PST),
                            ("RoundRobin_GF_off_allowed", pst, PST)):
    for seed in (71, 72):
        env = EV2Gym(config_file=cfg, seed=seed, state_function=getattr(S, sf), reward_function=getattr(RW, rf), generate_rnd_game=True)
        env.reset(seed=seed)
        ref, mine = getattr(H, name)(env=env), getattr(MINE, name)(env=env)
        assert ref.algo_name == mine.algo_name
        moved = 0
        for t in range(env.simulation_length):
            a, b = ref.get_action(env), mine.get_action(env)
            assert np.array_equal(a, b), (name, seed, t, a, b)
            moved += int((a != a.min()).sum())
            env.step(a.copy())
        assert moved > 0, (name, seed)
print("OK")
"""


def test_new_facade_agents_equal_the_reference_agents_step_by_step(tmp_path):
    """Two short reference episodes per agent: the reference's agent and the facade agent read the SAME reference env in lockstep and choose
    the same actions bit for bit.  Needs a checkout of the upstream reference (not part of this repository); in its own process because
    the import shim installs module stubs and changes the working directory."""
    from oracle.ref_import import REF_ROOT
    if not os.path.isdir(os.path.join(REF_ROOT, "ev2gym")):
        pytest.skip(f"no checkout of the upstream reference at {REF_ROOT} (not part of this repository)")
    r = subprocess.run([sys.executable, "-c", _LOCKSTEP, ROOT], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-3000:])


def test_new_heuristic_kernels_compile_without_spills_or_scratch(tmp_path):
    """Kinds 3-5 of ev2g_heuristic_kernel inside the budget tests/test_heuristics_cpu.py holds kinds 0-2 to (the compiler's own figures,
    -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
    from ev2gym_amd import build
    src = tmp_path / "heur.hip"
    src.write_text('#include "ev2g_heuristic.h"\n' + "".join(
        f"template __global__ void ev2g_heuristic_kernel<{k}>(DevScn, DevState, HeurArgs, int, double *);\n" for k in (3, 4, 5)))
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
        print(k, v)
        assert v["VGPRs"] <= 64 and v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
