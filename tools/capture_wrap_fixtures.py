#!/usr/bin/env python3
"""Captures the `wrap_*` fixtures of the reference's action wrappers (rl_agent/action_wrappers.py: BinaryAction, ThreeStep_Action,
Rescale_RepairLayer) with oracle/capture_golden.run_case: the live reference env is driven through the reference's own wrapper objects --
`wrapper.action(a)` before `env.step`, which is all gymnasium's ActionWrapper does -- and the raw and wrapped actions are recorded next to the
usual trajectory.  The fixture's `act` / `trj_*` are the WRAPPED actions and what the env made of them, so every fixture is also an ordinary
step fixture.  For the repair layer the wrapper's inputs of every step are recorded too (per port: an EV is connected, its current and
battery capacity, its AC power limits; the step's setpoint), so that ev2gym_amd.rl_agent.action_wrappers.WrapModel can be replayed without an
env; the tool replays it, asserts the wrapped actions bit for bit and prints which branch each step took.

Needs a checkout of the upstream reference where oracle/ref_import.py expects it, on an interpreter older than CPython 3.12 (later ones
compensate sum() over floats, which the reference's wrapper was not written for).  Writes tests/golden/wrap/<name>.npz (EV2G_GOLDEN_OUT
redirects, as for oracle/capture_golden.py); names given on the command line select cases.

    python tools/capture_wrap_fixtures.py [name ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # capture_golden imports its siblings by their bare names
sys.path.insert(1, ROOT)

import capture_golden as cg  # noqa: E402

if not os.environ.get("EV2G_GOLDEN_OUT"):
    cg.OUT = os.path.join(cg.OUT, "wrap")   # tests/golden/ itself is globbed by existing tests

PPL = ("V2G_profit_max_loads", "ProfitMax_TrPenalty_UserIncentives")
PST = ("PublicPST", "SquaredTrackingErrorReward")


def port_state(env):
    """What Rescale_RepairLayer.update_ev_buffer reads of every port, in the reference's port order."""
    rows = []
    for cs in env.charging_stations:
        for ev in cs.evs_connected:
            rows.append((0.0, 0.0, 1.0, 0.0, 0.0) if ev is None else
                        (1.0, ev.current_capacity, ev.battery_capacity, ev.min_ac_charge_power, ev.max_ac_charge_power))
    return np.array(rows, np.float64)


class Driven:
    """The reference env as run_case drives it, with the reference's wrapper object in the loop and raw actions of this tool's own."""

    def __init__(self, env, wrapper, draw):
        self.__dict__.update(env=env, wrapper=wrapper, draw=draw, rec=dict(raw=[], act=[], state=[], setpoint=[]))

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kw):
        return self.env.reset(**kw)

    def step(self, a):
        raw = self.draw(len(a))
        self.rec["raw"].append(raw.copy())
        self.rec["state"].append(port_state(self.env))
        self.rec["setpoint"].append(float(self.env.power_setpoints[self.env.current_step]))
        d = np.array(self.wrapper.action(raw.copy()), np.float64)
        self.rec["act"].append(d.copy())
        out = self.env.step(d)
        a[:] = d   # run_case records the caller's array after the step: what the env left of the wrapped actions
        return out


def cases():
    base = "ev2gym/example_config_files/"
    ppl, pst = base + "V2GProfitPlusLoads.yaml", base + "PublicPST.yaml"
    p2 = cg._yaml_variant(ppl, {"number_of_charging_stations": 12, "number_of_ports_per_cs": 2}, "wrap_v2gppl_p2")
    busy = cg._yaml_variant(pst, {"spawn_multiplier": 10}, "wrap_pst_busy")
    ppl_sp = cg._yaml_variant(ppl, {"power_setpoint_enabled": True}, "wrap_v2gppl_sp")
    # eight one-port chargers of unequal power on one transformer: the queue position's charger differs from the entry's own
    topo = cg._topology_file("wrap_unequal", [(400, [(1, 32, 0, 400, 3), (1, 16, 0, 230, 1), (1, 32, 0, 230, 3), (1, 16, 0, 400, 3),
                                                     (1, 32, 0, 400, 1), (1, 16, 0, 230, 3), (1, 32, 0, 230, 1), (1, 16, 0, 400, 1)])])
    uneq = cg._yaml_variant(pst, {"charging_network_topology": topo, "spawn_multiplier": 10}, "wrap_pst_unequal")
    #       name, config, kinds, seed, wrapper class, raw actions
    return [("wrap_binary_v2gppl_p2_s71", p2, PPL, 71, "BinaryAction", "uniform"),
            ("wrap_threestep_pst_s72", pst, PST, 72, "ThreeStep_Action", "levels"),
            ("wrap_repair_pst_s5", pst, PST, 5, "Rescale_RepairLayer", "uniform"),
            ("wrap_repair_pst_busy_s5", busy, PST, 5, "Rescale_RepairLayer", "uniform"),
            ("wrap_repair_v2gppl_sp_s5", ppl_sp, PPL, 5, "Rescale_RepairLayer", "uniform"),
            ("wrap_repair_pst_unequal_s5", uneq, PST, 5, "Rescale_RepairLayer", "uniform")]


def replay(z):
    """WrapModel on a fixture's recorded inputs: the wrapped actions [T, P] and, for the repair layer, each step's branch and whether some
    queue position's charger power differed from its port's."""
    from ev2gym_amd.rl_agent.action_wrappers import WrapModel
    name = str(z["wrap_class"])
    T, P = z["wrap_raw"].shape
    m = WrapModel(name, 1, P, z["wrap_min_action"], z["wrap_cs_kw"], z["wrap_cs_min_kw"])
    out, branch, mismatch = np.zeros((T, P)), np.zeros(T, np.int64), np.zeros(T, bool)
    for t in range(T):
        if name == "Rescale_RepairLayer":
            st = z["wrap_state"][t]
            out[t] = m.action(z["wrap_raw"][t], st[:, 0] != 0, st[:, 1], st[:, 2], st[:, 3], st[:, 4], z["wrap_setpoint"][t:t + 1])[0]
            branch[t], mismatch[t] = m.branch[0], m.mismatch[0]
        else:
            out[t] = m.action(z["wrap_raw"][t])[0]
    return out, branch, mismatch


def run(name, config, kinds, seed, cls, raw):
    from ev2gym.models.ev2gym_env import EV2Gym
    import ev2gym.rl_agent.action_wrappers as AW
    import ev2gym.rl_agent.reward as RW
    import ev2gym.rl_agent.state as S
    from ev2gym_amd.rl_agent.action_wrappers import charger_tables
    env = EV2Gym(config_file=config, seed=seed, state_function=getattr(S, kinds[0]), reward_function=getattr(RW, kinds[1]),
                 generate_rnd_game=True)
    wrapper = getattr(AW, cls)(env)
    rng = np.random.default_rng(seed)
    draw = (lambda n: rng.uniform(0.0, 1.0, n)) if raw == "uniform" else (lambda n: rng.integers(0, 3, n).astype(np.float64))
    drv = Driven(env, wrapper, draw)
    cg.run_case(name, config, *kinds, seed, "rand", None, env=drv)
    path = os.path.join(cg.OUT, name + ".npz")
    z = dict(np.load(path))
    rec = {k: np.array(v) for k, v in drv.rec.items()}
    z["act"] = rec["act"]
    arrs = {k[4:]: v for k, v in z.items() if k.startswith("scn_cs_")}
    arrs.setdefault("cs_n_ports", np.full(len(arrs["cs_voltage"]), int(z["scn_meta"][3])))
    tabs = charger_tables(arrs)
    assert np.array_equal(tabs[0], np.asarray(wrapper.min_action).reshape(-1))
    z.update(wrap_class=np.array(cls), wrap_raw=rec["raw"], wrap_act=rec["act"], wrap_min_action=tabs[0], wrap_cs_kw=tabs[1], wrap_cs_min_kw=tabs[2])
    if cls == "Rescale_RepairLayer":
        assert np.array_equal(tabs[1], wrapper.max_cs_power)
        z.update(wrap_state=rec["state"], wrap_setpoint=rec["setpoint"])
    np.savez_compressed(path, **z)
    z = np.load(path)
    out, branch, mismatch = replay(z)
    assert np.array_equal(out, z["wrap_act"]), (name, np.nonzero((out != z["wrap_act"]).any(axis=1))[0][:5])
    print(f"{name}: changed {float((rec['act'] != rec['raw']).mean()):.3f} of the actions, branches pass/raise/raise-no-range/reduce/top-up "
          f"{np.bincount(branch, minlength=5).tolist()}, position != port in {int(mismatch.sum())} steps, {os.path.getsize(path) / 1024:.0f} KB",
          flush=True)


def main():
    cg.import_reference()
    only = set(sys.argv[1:])
    for c in cases():
        if not only or c[0] in only:
            run(*c)


if __name__ == "__main__":
    main()
