"""The reference's env-reading heuristic agents (RoundRobin, ChargeAsLateAsPossible, ChargeAsFastAsPossibleToDesiredCapacity;
baselines/heuristics.py) computed on the device from the engine's state (csrc/ev2g_heuristic.h, ev2g_heuristic_*): the actions of the
reference's own agents on its fixtures, of the facade agents on randomised scenarios, bit for bit, through every layer above the kernel."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden

pytestmark = pytest.mark.gpu

AGENT_FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("agent_"))
NAMES = ("ChargeAsLateAsPossible", "ChargeAsFastAsPossibleToDesiredCapacity", "RoundRobin")
DEFAULT_KINDS = ("ProfitMax_TrPenalty_UserIncentives", "V2G_profit_max_loads")
PST_KINDS = ("SquaredTrackingErrorReward", "PublicPST")


def _engine(batch, kinds, **kw):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    kw.setdefault("flags", _abi.FLAG_LOG_SOC)
    return Engine(batch, _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], device=0, **kw)


def _episode(eng, agent, offset=None):
    """One episode of (agent's actions on the device -> step), every output copied out: actions [T,E,P], obs [T+1,E,D], reward [T,E], mask [T,E,P]."""
    E, P, D = eng.E, eng.P, eng.D
    act, obs, rew = eng.empty((E, P)), eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.reset(obs, offset=offset)
    out = dict(act=[], obs=[obs.to_host().copy()], rew=[], mask=[])
    for _ in range(eng.T):
        eng.heuristic_actions(agent, act)
        out["act"].append(act.to_host().copy())
        eng.step(act, obs, rew, done, mask)
        out["obs"].append(obs.to_host().copy())
        out["rew"].append(rew.to_host().copy())
        out["mask"].append(mask.to_host().copy())
    assert done.to_host().all()
    for b in (act, obs, rew, done, mask):
        b.free()
    return {k: np.array(v) for k, v in out.items()}


def _facade_actions_match(scenario, name, device_actions, kinds):
    """The facade agent of `name` on the one-env `scenario` chooses `device_actions` [T,P] at every step."""
    from ev2gym_amd import _abi
    from ev2gym_amd.baselines import heuristics as H
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.env import EV2Gym
    env = EV2Gym(scenario=scenario, state_function=kinds[1], reward_function=kinds[0])
    agent = getattr(H, name)(env=env)
    env.reset()
    try:
        for t in range(env.simulation_length):
            a = agent.get_action(env)
            assert np.array_equal(a, device_actions[t]), f"{name} step {t}: facade {a} device {device_actions[t]}"
            try:
                env.step(a)
            except EngineError as e:   # the reference's charger over-current exception (ev_charger.py:203-205): its episode ends here
                assert e.code == _abi.ERR_OVERCURRENT
                return
    finally:
        env.close()


def _kinds_for(batch):
    pst = bool(batch.arrays["power_setpoints"].any()) and batch.n_transformers == 1 and int(np.max(batch.arrays["cs_n_ports"])) == 1
    return PST_KINDS if pst else DEFAULT_KINDS


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("name", AGENT_FIXTURES)
def test_device_agents_choose_the_reference_actions(name, tile):
    """The agent_* fixtures record the actions the reference's agent chose at every step of a reference episode: the device agent chooses
    them bit for bit, and the trajectory it drives matches the fixture's (observations / rewards to 1e-9, masks exactly) -- on one env
    and on 64 copies of it."""
    z, batch, rk, sk = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    agent = str(z["case"][5]).split(":")[1]
    eng = _engine(batch.tile(tile) if tile > 1 else batch, (str(z["case"][3]), str(z["case"][2])))
    ep = _episode(eng, eng.heuristic_create(agent))
    eng.close()
    assert len(ep["act"]) == len(z["act"])
    for t in range(len(z["act"])):
        for e in range(tile):
            assert np.array_equal(ep["act"][t, e], z["act"][t]), f"step {t} env {e}: device {ep['act'][t, e]} reference {z['act'][t]}"
            ref = z["trj_obs"][t + 1]
            assert (np.abs(ep["obs"][t + 1, e] - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-9
            assert abs(ep["rew"][t, e] - z["trj_reward"][t]) <= 1e-9 * max(1.0, abs(z["trj_reward"][t]))
            assert (ep["mask"][t, e] == z["trj_mask"][t]).all()


@pytest.mark.parametrize("case", range(20))
def test_randomised_device_agents_equal_the_facade_agents(case):
    """Shapes, timescales, multi-port chargers and topology files drawn like tests/test_fuzz_gpu.py, 8 envs: for every env and agent the
    device's actions of every step are those of the facade agent on that env alone."""
    from ev2gym_amd.scenario_gen import generate
    from tests.test_fuzz_gpu import _draw
    _, cfg = _draw(700 + case)
    batch = generate(dataclasses.replace(cfg, n_envs=8))
    if batch.n_sessions == 0:
        pytest.skip("a draw without sessions")
    kinds = _kinds_for(batch)
    for name in NAMES:
        eng = _engine(batch, kinds)
        ep = _episode(eng, eng.heuristic_create(name))
        eng.close()
        for e in range(batch.n_envs):
            _facade_actions_match(batch.select([e]), name, ep["act"][:, e], kinds)


@pytest.mark.parametrize("shape", ["cfg4", "cfg3"])
def test_device_agents_equal_the_facade_agents_at_the_benchmark_shapes(shape):
    """cfg4's shape (1000 chargers, 50 transformers: stepped by ev2g_step_big) and cfg3's (PublicPST, two envs per wavefront)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    if shape == "cfg4":
        batch, kinds = generate(GenConfig.v2g_profit_plus_loads(2, 1000, 50, seed=41, power_setpoint_enabled=True)), DEFAULT_KINDS
    else:
        batch, kinds = generate(GenConfig.public_pst(8, 20, seed=42)), PST_KINDS
    for name in NAMES:
        eng = _engine(batch, kinds)
        ep = _episode(eng, eng.heuristic_create(name))
        if shape == "cfg4":
            assert eng.last_launch_specialisation == 5, "the cfg4 shape is expected on ev2g_step_big"
        eng.close()
        assert np.abs(ep["act"]).sum() > 0
        for e in range(batch.n_envs):
            _facade_actions_match(batch.select([e]), name, ep["act"][:, e], kinds)


@pytest.mark.parametrize("kinds", [DEFAULT_KINDS, PST_KINDS])
def test_heuristic_run_equals_the_step_by_step_loop(kinds):
    """ev2g_heuristic_run(k) with every output kept equals k x (heuristic_actions -> step) bit for bit -- over a whole episode and as two
    half-episode segments; a segment that would cross the episode end is refused before anything is launched."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate
    gen = (GenConfig.v2g_profit_plus_loads(16, 30, 1, seed=5, power_setpoint_enabled=True) if kinds == DEFAULT_KINDS
           else GenConfig.public_pst(16, 20, seed=6))
    batch = generate(gen)
    for name in NAMES:
        eng = _engine(batch, kinds)
        E, P, D, T = eng.E, eng.P, eng.D, eng.T
        ref = _episode(eng, eng.heuristic_create(name))
        a = eng.heuristic_create(name)
        bufs = dict(act=eng.empty((T, E, P)), obs=eng.empty((T, E, D)), rew=eng.empty((T, E)), done=eng.empty((T, E), np.uint8),
                    mask=eng.empty((T, E, P), np.uint8))
        for split in (T, T // 2):
            eng.reset()
            for t0, k in ((0, split), (split, T - split)):
                if k == 0:
                    continue
                b = {n: x.at(t0 * int(np.prod(x.shape[1:]))) for n, x in bufs.items()}
                eng.heuristic_run(a, k, b["act"], E * P, b["obs"], E * D, b["rew"], E, b["done"], E, b["mask"], E * P)
            assert eng.last_step_n_kernel_ms() > 0
            got = {n: x.to_host() for n, x in bufs.items()}
            assert np.array_equal(got["act"], ref["act"]), (name, split)
            assert np.array_equal(got["obs"], ref["obs"][1:]), (name, split)
            assert np.array_equal(got["rew"], ref["rew"]), (name, split)
            assert np.array_equal(got["mask"], ref["mask"]), (name, split)
            assert got["done"][-1].all() and not got["done"][:-1].any()
        eng.reset()
        eng.heuristic_run(a, T // 2)   # actions into the agent's own buffer
        with pytest.raises(EngineError) as ei:
            eng.heuristic_run(a, T - T // 2 + 1)
        assert ei.value.code == _abi.ERR_DONE and eng.current_step == T // 2
        eng.close()


def test_round_robin_starts_every_episode_with_an_empty_queue():
    """EV2GymVec with auto-reset and ONE RoundRobin(env=vec) across two episodes: the second episode's actions are those of a fresh agent
    on the scenarios it ran (the reference builds a fresh agent for every run, evaluator.py:237)."""
    from ev2gym_amd.baselines.heuristics import RoundRobin
    from ev2gym_amd.scenario_gen import GenConfig, generate
    from ev2gym_amd.vec_env import EV2GymVec
    E = 8
    pool = generate(GenConfig.public_pst(2 * E, 20, seed=8))
    vec = EV2GymVec(scenarios=pool, num_envs=E, state_function=PST_KINDS[1], reward_function=PST_KINDS[0], auto_reset=True, use_torch=False,
                    seed=3)
    agent = RoundRobin(env=vec)
    eps = []
    for _ in range(2):
        off, acts = vec.engine.scenario_offset, []
        for _ in range(vec.simulation_length):
            a = agent.get_action(vec)
            acts.append(a.to_host().copy())
            vec.step(a)
        eps.append((off, np.array(acts)))
    vec.close()
    assert eps[0][0] != eps[1][0], "auto-reset moves the envs onto another window of the pool"
    for off, acts in eps:
        eng = _engine(pool, PST_KINDS, n_active_envs=E)
        fresh = _episode(eng, eng.heuristic_create("RoundRobin"), offset=off)
        eng.close()
        assert np.array_equal(acts, fresh["act"])


@pytest.mark.parametrize("case", [0, 3])
def test_device_agents_on_a_device_refilled_pool(case):
    """A pool refilled on the device (ev2g_pool_refill: no host copy of the scenarios exists) runs every agent's episode exactly like a pool
    loaded from the host-generated scenarios (the pattern of test_randomised_device_refill_equals_the_host_generator)."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import generate_native
    from tests.test_fuzz_gpu import _draw
    _, cfg = _draw(500 + case)
    M, S1 = 12, int(cfg.seed)
    mk = lambda n, seed: dataclasses.replace(cfg, n_envs=n, seed=seed)   # noqa: E731
    host, other = generate_native(mk(M + 5, S1)), generate_native(mk(M, S1 + 7919))
    if host.n_sessions == 0 or other.n_sessions == 0:
        pytest.skip("a draw without sessions")
    kinds = _kinds_for(host)
    flags = _abi.FLAG_LOG_SOC | _abi.FLAG_REFILLABLE
    eng = _engine(other, kinds, flags=flags)
    try:
        eng.pool_refill(mk(M, S1), S1, 3, 0, M)
    except EngineError as e:
        eng.close()
        pytest.skip(f"outside the device generator's stated limits: {e}")
    if eng.pool_refill_overflows:
        eng.close()
        pytest.skip("the refilled scenarios draw more sessions than the loaded pool's blocks hold")
    got = {n: _episode(eng, eng.heuristic_create(n)) for n in NAMES}
    eng.close()
    ref_eng = _engine(host.select(np.arange(3, M + 3)), kinds, flags=flags)
    ref = {n: _episode(ref_eng, ref_eng.heuristic_create(n)) for n in NAMES}
    ref_eng.close()
    assert np.abs(ref["ChargeAsFastAsPossibleToDesiredCapacity"]["act"]).sum() > 0
    for n in NAMES:
        for k in ("act", "obs", "rew", "mask"):
            assert np.array_equal(got[n][k], ref[n][k]), (n, k)


def test_evaluator_runs_the_env_reading_agents_on_the_device():
    """evaluate(..., algorithms=DEVICE_HEURISTICS): one row per (run, algorithm), each row the statistics of the facade agent's episode on that
    run alone (to 1e-9); the default call still returns exactly the three closed-form algorithms."""
    from ev2gym_amd.baselines import heuristics as H
    from ev2gym_amd.env import EV2Gym
    from ev2gym_amd.evaluator import ALGORITHMS, DEVICE_HEURISTICS, RESULT_STATS, evaluate
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(16, 10, 1, seed=9, power_setpoint_enabled=True))
    df = evaluate(batch, algorithms=list(DEVICE_HEURISTICS), seed=1)
    assert len(df) == 16 * len(DEVICE_HEURISTICS) and list(df["Algorithm"].unique()) == list(DEVICE_HEURISTICS)
    assert (df["time"] > 0).all()
    for name in DEVICE_HEURISTICS:
        sub = df[df["Algorithm"] == name].sort_values("run")
        assert sub["run"].tolist() == list(range(16))
        for e in range(16):
            env = EV2Gym(scenario=batch.select([e]), state_function=DEFAULT_KINDS[1], reward_function=DEFAULT_KINDS[0])
            agent = getattr(H, name)(env=env)
            env.reset()
            done = False
            while not done:
                _, _, done, _, _ = env.step(agent.get_action(env))
            for k in RESULT_STATS + ["total_reward"]:
                got, want = float(sub[k].iloc[e]), float(env.stats[k])
                assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-9 * max(1.0, abs(want)), (name, e, k, got, want)
            env.close()
    assert sorted(evaluate(batch.select(np.arange(4)))["Algorithm"].unique()) == sorted(ALGORITHMS)


def test_device_agents_keep_a_rate_floor_at_cfg2():
    """Regression guard only: 4096 envs x 50 chargers, one whole episode per agent through heuristic_run, at >= 20 M env-steps/s of kernel
    time (the facade walks the object graph at ~5 k)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    batch = generate_native(GenConfig.v2g_profit_plus_loads(4096, 50, 1, seed=11, power_setpoint_enabled=True))
    eng = _engine(batch, DEFAULT_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    for name in NAMES:
        a = eng.heuristic_create(name)
        for _ in range(2):   # warm-up episode, then the timed one
            eng.reset()
            eng.heuristic_run(a, T, None, 0, obs, 0, rew, 0, done, 0, mask, 0)
            rate = E * T / (eng.last_step_n_kernel_ms() / 1e3)
        eng.check_faults()
        assert rate >= 20e6, (name, rate)
    eng.close()
