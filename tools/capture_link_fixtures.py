#!/usr/bin/env python3
"""Captures the `link_*` fixtures of the reference's two communication-fault wrappers (rl_agent/noise_wrappers.py: FailedActionCommunication,
DelayedObservation) with oracle/capture_golden.run_case: the live reference env is driven through the reference's own wrapper objects --
`wrapper.action(a)` before `env.step`, `wrapper.observation(obs)` on the reset observation and on every step's, which is all gymnasium's
wrapper base classes do -- and the wrapper's uniforms, the raw and delivered actions and the raw and delivered observations are recorded next
to the usual trajectory.  The fixture's `act` / `trj_*` are the DELIVERED actions and the env's own (raw) observations, so every fixture is
also an ordinary step fixture.  The delay fixtures stop one step short of the episode end: at the terminal observation the reference indexes
its [P, T] matrix out of range.

Needs a checkout of the upstream reference where oracle/ref_import.py expects it.  Writes tests/golden/<name>.npz (EV2G_GOLDEN_OUT
redirects, as for oracle/capture_golden.py); names given on the command line select cases.

    python tools/capture_link_fixtures.py [name ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # capture_golden imports its siblings by their bare names
sys.path.insert(1, ROOT)

import capture_golden as cg  # noqa: E402

PPL = ("V2G_profit_max_loads", "ProfitMax_TrPenalty_UserIncentives")
PST = ("PublicPST", "SquaredTrackingErrorReward")
P_HIT = 0.3


class Driven:
    """The reference env as run_case drives it, with the reference's wrapper objects in the loop."""

    def __init__(self, env, fail, delay):
        self.__dict__.update(env=env, fail=fail, delay=delay, rec=dict(raw_act=[], act=[], raw_obs=[], obs=[]))

    def __getattr__(self, name):
        return getattr(self.env, name)

    def _observe(self, obs):
        self.rec["raw_obs"].append(np.array(obs, np.float64))
        self.rec["obs"].append(np.array(self.delay.observation(np.array(obs, np.float64)) if self.delay else obs, np.float64))

    def reset(self, **kw):
        obs, info = self.env.reset(**kw)
        self._observe(obs)
        return obs, info

    def step(self, a):
        self.rec["raw_act"].append(a.copy())
        d = self.fail.action(a) if self.fail else a.copy()
        self.rec["act"].append(d.copy())
        out = self.env.step(d)
        a[:] = d   # run_case records the caller's array after the step: what the env left of the delivered commands
        self._observe(out[0])
        return out


def cases():
    base = "ev2gym/example_config_files/"
    ppl, pst = base + "V2GProfitPlusLoads.yaml", base + "PublicPST.yaml"
    busy = cg._yaml_variant(pst, {"spawn_multiplier": 10}, "link_pst_busy")   # most slots occupied: the delay has something to delay
    #       name, config, kinds, seed, p_fail, p_delay
    return [("link_fail_v2gppl_s81", ppl, PPL, 81, P_HIT, 0.0),
            ("link_fail_pst_s82", pst, PST, 82, P_HIT, 0.0),
            ("link_delay_pst_s83", busy, PST, 83, 0.0, P_HIT),
            ("link_both_pst_s84", busy, PST, 84, P_HIT, P_HIT)]


def run(name, config, kinds, seed, p_fail, p_delay):
    from ev2gym.models.ev2gym_env import EV2Gym
    import ev2gym.rl_agent.noise_wrappers as NW
    import ev2gym.rl_agent.reward as RW
    import ev2gym.rl_agent.state as S
    env = EV2Gym(config_file=config, seed=seed, state_function=getattr(S, kinds[0]), reward_function=getattr(RW, kinds[1]),
                 generate_rnd_game=True)
    np.random.seed(seed)   # the wrappers draw their matrices from numpy's global generator at construction
    fail = NW.FailedActionCommunication(env, p_fail=p_fail) if p_fail > 0 else None
    delay = NW.DelayedObservation(env, p_delay=p_delay) if p_delay > 0 else None   # (both wrappers read env.unwrapped only: stacking changes nothing)
    drv = Driven(env, fail, delay)
    steps = env.simulation_length - 1 if delay else None
    cg.run_case(name, config, *kinds, seed, "rand", steps, env=drv)
    path = os.path.join(cg.OUT, name + ".npz")
    z = dict(np.load(path))
    rec = {k: np.array(v) for k, v in drv.rec.items()}
    assert np.array_equal(z["act"], rec["raw_act"]) and np.array_equal(z["trj_obs"], rec["raw_obs"])
    z["act"] = rec["act"]
    z.update(link_raw_act=rec["raw_act"], link_act=rec["act"], link_raw_obs=rec["raw_obs"], link_obs=rec["obs"],
             link_p=np.array([p_fail, p_delay]), link_rand_act=fail.random if fail else np.zeros((0, 0)),
             link_rand_obs=delay.random if delay else np.zeros((0, 0)))
    np.savez_compressed(path, **z)
    held = float((rec["act"] != rec["raw_act"]).mean())
    late = float((rec["obs"] != rec["raw_obs"])[:, 4::3].mean()) if delay else 0.0
    print(f"{name}: held {held:.3f} of the commands, delayed {late:.3f} of the energy columns, {os.path.getsize(path) / 1024:.0f} KB", flush=True)


def import_reference():
    """oracle's import of the reference, plus what its noise_wrappers module needs of a gymnasium stand-in: ObservationWrapper and Env are
    subscripted there (Generics in gymnasium proper)."""
    cg.import_reference()
    gym = sys.modules["gymnasium"]
    for name, parent in (("ObservationWrapper", gym.Wrapper), ("Env", gym.Env)):
        if not hasattr(getattr(gym, name), "__class_getitem__"):
            setattr(gym, name, type(name, (parent,), {"__class_getitem__": classmethod(lambda cls, item: cls)}))


def main():
    import_reference()
    only = set(sys.argv[1:])
    for c in cases():
        if not only or c[0] in only:
            run(*c)


if __name__ == "__main__":
    main()
