"""The reference's three later env-reading agents on the device (kinds 3-5 of csrc/ev2g_heuristic.h: ChargeAsLateAsPossibleToDesiredCapacity,
RoundRobin_GF, RoundRobin_GF_off_allowed): the device's actions against the facade agents' (ev2gym_amd/baselines/heuristics.py, themselves held
to the reference's by the agent_* fixtures and tests/test_agents_more_cpu.py) bit for bit, at every step, through every layer above the kernel."""
import dataclasses

import numpy as np
import pytest

from tests.test_heuristics_gpu import DEFAULT_KINDS, PST_KINDS, _engine, _episode, _kinds_for

pytestmark = pytest.mark.gpu

CALPDC, GF, GF_OFF = NEW = ("ChargeAsLateAsPossibleToDesiredCapacity", "RoundRobin_GF", "RoundRobin_GF_off_allowed")
# draws of tests/test_fuzz_gpu._draw, chosen on the CPU: all nine have sessions; 902, 903, 908, 912, 914 and 923 have one-port chargers only
# (903, 912, 914, 923 with power setpoints), 911, 913 and 917 have chargers with three or four ports
FUZZ_SEEDS = (902, 903, 908, 911, 912, 913, 914, 917, 923)


def _one_port(batch):
    return int(np.max(batch.arrays["cs_n_ports"])) == 1


def _facade_episode(scenario, name, device_actions, kinds, probe=None):
    """The facade agent `name` on the one-env `scenario` chooses `device_actions` [T,P] at every step; probe(agent, env, t) sees the agent
    after each choice.  Ends like the reference where its charger over-current exception ends the episode."""
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
            if probe is not None:
                probe(agent, env, t)
            try:
                env.step(a)
            except EngineError as e:
                assert e.code == _abi.ERR_OVERCURRENT
                return
    finally:
        env.close()


def _device_equals_facade(batch, names, kinds, probe=None, **kw):
    for name in names:
        eng = _engine(batch, kinds, **kw)
        ep = _episode(eng, eng.heuristic_create(name))
        eng.close()
        for e in range(batch.n_envs):
            _facade_episode(batch.select([e]), name, ep["act"][:, e], kinds, (lambda *a, n=name, e=e: probe(n, e, *a)) if probe else None)


def _fuzz_batch(seed):
    from ev2gym_amd.scenario_gen import generate
    from tests.test_fuzz_gpu import _draw
    return generate(dataclasses.replace(_draw(seed)[1], n_envs=8))


def test_the_randomised_draws_cover_both_charger_layouts():
    batches = [_fuzz_batch(s) for s in FUZZ_SEEDS]
    with_sessions = [b for b in batches if b.n_sessions > 0]
    assert len(with_sessions) >= 6 and sum(_one_port(b) for b in with_sessions) >= 4
    assert any(not _one_port(b) for b in with_sessions)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_randomised_device_agents_equal_the_facade_agents(seed):
    """Shapes, timescales, multi-port chargers and topology files drawn like tests/test_fuzz_gpu.py, 8 envs: kind 3 on every draw, kinds 4 and
    5 on the draws whose chargers all have one port."""
    batch = _fuzz_batch(seed)
    assert batch.n_sessions > 0
    _device_equals_facade(batch, NEW if _one_port(batch) else (CALPDC,), _kinds_for(batch))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_round_robin_gf_queues_across_the_64_entry_chunks(P):
    """One wavefront walks the queue 64 entries at a time: port counts around one and two chunks, non-zero minimum powers (the GF total starts
    from their sum), a setpoint that serves a few EVs per step so that the queue stays long."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.public_pst(4, P, seed=30 + P, scenario="workplace", spawn_multiplier=10, cs_min_charge_current=6.0,
                                          power_setpoint_flexiblity=20.0))
    assert batch.n_transformers == 1 and batch.arrays["power_setpoints"].any()
    longest = {}

    def probe(name, e, agent, env, t):
        longest[name] = max(longest.get(name, 0), len(agent.ev_buffer))
        assert len(agent.ev_buffer) == len(agent.min_power) == len(agent.max_power)

    _device_equals_facade(batch, (GF, GF_OFF), PST_KINDS, probe)
    print("longest queue", P, longest)
    if P == 130:
        assert min(longest.values()) > 64, longest


def _queue_totals(scenario, name, kinds):
    """One facade episode of a RoundRobin_GF agent: per step, the queue length and the total the agent would reach by taking the WHOLE queue
    (its own sequential sums), read after update_ev_buffer and before the choice."""
    from ev2gym_amd.baselines import heuristics as H
    from ev2gym_amd.env import EV2Gym
    env = EV2Gym(scenario=scenario, state_function=kinds[1], reward_function=kinds[0])
    agent = getattr(H, name)(env=env)
    env.reset()
    out = []
    for t in range(env.simulation_length):
        agent.update_ev_buffer(env)   # (get_action repeats it: nothing changes the second time)
        total = 0
        if not agent.off_allowed:
            for lo in agent.min_power:
                total += lo
        for lo, hi in zip(agent.min_power, agent.max_power):
            total += hi if agent.off_allowed else hi - lo
        out.append((len(agent.ev_buffer), float(total)))
        env.step(agent.get_action(env))
    env.close()
    return out


@pytest.mark.parametrize("name", [GF, GF_OFF])
def test_round_robin_gf_at_the_setpoint_edges(name):
    """A hand-edited batch: at one step env 0's setpoint is EXACTLY the total of its whole queue (RoundRobin_GF's `>=` trims the last EV
    by 0 / max power, the off-allowed variant's strict `>` does not trim: both leave it at 1 and every queued EV charges), three steps
    later every env's setpoint is 0 (one EV is chosen and trimmed by its whole range).  A setpoint only decides the choice of ITS step, so
    the queue the edit was computed from is the queue the edited episode has there."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    base = generate(GenConfig.public_pst(4, 12, seed=77, spawn_multiplier=10, cs_min_charge_current=4.0))   # (below every EV's maximum power)
    totals = _queue_totals(base.select([0]), name, PST_KINDS)
    t_eq = next(t for t, (n, _) in enumerate(totals) if t >= 5 and n >= 3)
    t_zero = t_eq + 3
    batch = base.select(np.arange(4))
    sp = batch.arrays["power_setpoints"]
    sp[0, t_eq] = totals[t_eq][1]
    sp[:, t_zero] = 0.0
    assert base.arrays["power_setpoints"][0, t_eq] != sp[0, t_eq], "the edit must not reach the batch it was computed from"
    seen = {}

    def probe(_, e, agent, env, t):
        if e == 0 and t in (t_eq, t_zero):
            seen[t] = (len(agent.ev_buffer), env.power_setpoints[t])

    eng = _engine(batch, PST_KINDS)
    ep = _episode(eng, eng.heuristic_create(name))
    eng.close()
    for e in range(4):
        _facade_episode(batch.select([e]), name, ep["act"][:, e], PST_KINDS, lambda *a, e=e: probe(name, e, *a))
    assert seen[t_eq] == totals[t_eq] and seen[t_zero][1] == 0.0
    idle = 0.0 if name == GF_OFF else 4.0 / 16.0 + 1e-4
    a_eq, a_zero = ep["act"][t_eq, 0], ep["act"][t_zero]
    assert (a_eq == 1.0).sum() == totals[t_eq][0] and ((a_eq == 1.0) | (a_eq == idle)).all()   # the whole queue at 1, total == setpoint
    for e in range(4):   # setpoint 0: at most one EV off the idle level, trimmed below it or to (almost) nothing
        assert (a_zero[e] != idle).sum() <= 1 and (a_zero[e] < 1.0).all()


def test_round_robin_gf_keeps_a_queue_entrys_powers_across_back_to_back_sessions():
    """Stays extended up to the step before the port's next arrival (tests/test_fuzz_gpu._back_to_back): a port that is queued when its EV
    leaves stays queued for the next one, with the powers of the EV it was inserted for.  The mixed fleet's EVs differ in maximum power, and
    the facade agent is seen holding such a stale entry."""
    from ev2gym_amd.scenario import resolve_ports
    from ev2gym_amd.scenario_gen import GenConfig, generate
    from tests.test_fuzz_gpu import _back_to_back
    batch = generate(GenConfig.public_pst(4, 6, seed=53, spawn_multiplier=10))
    _back_to_back(batch)
    a, port = batch.arrays, resolve_ports(batch)
    assert any(a["ev_t_arr"][s] - 1 == a["ev_t_dep"][r] and port[s] == port[r] and a["ev_pac_max"][s] != a["ev_pac_max"][r]
               for r in range(batch.n_sessions - 1) for s in range(r + 1, min(r + 12, batch.n_sessions))
               if np.searchsorted(a["env_session_start"], r, "right") == np.searchsorted(a["env_session_start"], s, "right"))
    stale = {GF: 0, GF_OFF: 0}

    def probe(name, e, agent, env, t):
        for p, hi in zip(agent.ev_buffer, agent.max_power):
            cs = env.charging_stations[p]
            ev = cs.evs_connected[0]
            stale[name] += int(ev is not None and hi != min(cs.get_max_power(), ev.max_ac_charge_power))

    _device_equals_facade(batch, (GF, GF_OFF), PST_KINDS, probe)
    assert stale[GF] > 0 and stale[GF_OFF] > 0, stale


@pytest.mark.parametrize("name", NEW)
def test_new_device_agents_equal_the_facade_agents_at_cfg4s_shape(name):
    """2 envs x 1000 one-port chargers on 50 transformers with power setpoints (stepped by ev2g_step_big): the queue spans sixteen chunks."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(2, 1000, 50, seed=41, power_setpoint_enabled=True))
    eng = _engine(batch, DEFAULT_KINDS)
    ep = _episode(eng, eng.heuristic_create(name))
    assert eng.last_launch_specialisation == 5, "the cfg4 shape is expected on ev2g_step_big"
    eng.close()
    assert np.abs(ep["act"]).sum() > 0
    for e in range(batch.n_envs):
        _facade_episode(batch.select([e]), name, ep["act"][:, e], DEFAULT_KINDS)


@pytest.mark.parametrize("name", NEW)
def test_heuristic_run_equals_the_step_by_step_loop(name):
    """ev2g_heuristic_run(k) with every output kept equals k x (heuristic_actions -> step) bit for bit, over a whole episode and as two
    half-episode segments, 16 envs."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.public_pst(16, 20, seed=6, cs_min_charge_current=6.0, ev_desired_capacity=0.8))
    eng = _engine(batch, PST_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    ref = _episode(eng, eng.heuristic_create(name))
    assert len(np.unique(ref["act"])) > 3
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
        got = {n: x.to_host() for n, x in bufs.items()}
        assert np.array_equal(got["act"], ref["act"]), (name, split)
        assert np.array_equal(got["obs"], ref["obs"][1:]), (name, split)
        assert np.array_equal(got["rew"], ref["rew"]), (name, split)
        assert np.array_equal(got["mask"], ref["mask"]), (name, split)
        assert got["done"][-1].all() and not got["done"][:-1].any()
    eng.close()


def test_round_robin_gf_starts_every_episode_with_an_empty_queue():
    """EV2GymVec with auto-reset and ONE RoundRobin_GF(env=vec) across two episodes: the second episode's actions are those of a fresh agent on
    the scenarios it ran."""
    from ev2gym_amd.baselines.heuristics import RoundRobin_GF
    from ev2gym_amd.scenario_gen import GenConfig, generate
    from ev2gym_amd.vec_env import EV2GymVec
    E = 8
    pool = generate(GenConfig.public_pst(2 * E, 20, seed=8))
    vec = EV2GymVec(scenarios=pool, num_envs=E, state_function=PST_KINDS[1], reward_function=PST_KINDS[0], auto_reset=True, use_torch=False,
                    seed=3)
    agent = RoundRobin_GF(env=vec)
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
        fresh = _episode(eng, eng.heuristic_create(GF), offset=off)
        eng.close()
        assert np.array_equal(acts, fresh["act"])


def test_round_robin_gf_is_refused_for_multi_port_chargers():
    """The reference indexes a per-charger table with a port id: with two ports per charger kinds 4 and 5 are refused (EV2G_ERR_ARG, by name
    and by kind number), and the handle goes on to run kind 3."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(4, 5, 1, seed=12, number_of_ports_per_cs=2, ev_desired_capacity=0.8))
    eng = _engine(batch, DEFAULT_KINDS)
    for name in (GF, GF_OFF, 4, 5):
        with pytest.raises(EngineError) as ei:
            eng.heuristic_create(name)
        assert ei.value.code == -1 and "one port per charger" in str(ei.value)   # EV2G_ERR_ARG
    with pytest.raises(EngineError) as ei:
        eng.heuristic_create(6)
    assert ei.value.code == -1 and "unknown" in str(ei.value)
    assert _abi.AGENT_KINDS[CALPDC] == 3
    ep = _episode(eng, eng.heuristic_create(3))
    eng.close()
    assert np.abs(ep["act"]).sum() > 0
    for e in range(batch.n_envs):
        _facade_episode(batch.select([e]), CALPDC, ep["act"][:, e], DEFAULT_KINDS)


def test_a_reload_to_multi_port_chargers_stops_a_live_round_robin_gf_agent():
    """ev2g_load_scenarios under live agents, same envs and ports but 5 two-port chargers where 10 one-port chargers were: the kind-4 and
    kind-5 agents are refused from then on (EV2G_ERR_ARG; the kernel would index the charger table with a port id), nothing is launched
    and the step counter stays; a kind-3 agent of the same handle goes on and equals the facade on the new scenarios; loading one-port
    chargers again lets the GF agents run again."""
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate
    one = generate(GenConfig.v2g_profit_plus_loads(4, 10, 1, seed=13, power_setpoint_enabled=True, ev_desired_capacity=0.8))
    two = generate(GenConfig.v2g_profit_plus_loads(4, 5, 1, seed=14, number_of_ports_per_cs=2, power_setpoint_enabled=True,
                                                   ev_desired_capacity=0.8))
    assert one.n_ports == two.n_ports == 10 and one.n_envs == two.n_envs
    eng = _engine(one, DEFAULT_KINDS)
    agents = {n: eng.heuristic_create(n) for n in NEW}
    act = eng.empty((eng.E, eng.P))
    eng.reset()
    for n in NEW:
        eng.heuristic_actions(agents[n], act)
    eng.load(two)
    eng.reset()
    for n in (GF, GF_OFF):
        for call in (lambda: eng.heuristic_actions(agents[n], act), lambda: eng.heuristic_run(agents[n], 1)):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == -1 and "one port per charger" in str(ei.value)   # EV2G_ERR_ARG
    assert eng.current_step == 0
    act.free()
    ep = _episode(eng, agents[CALPDC])
    assert np.abs(ep["act"]).sum() > 0
    for e in range(two.n_envs):
        _facade_episode(two.select([e]), CALPDC, ep["act"][:, e], DEFAULT_KINDS)
    eng.load(one)
    ep = _episode(eng, agents[GF])
    eng.close()
    for e in range(one.n_envs):
        _facade_episode(one.select([e]), GF, ep["act"][:, e], DEFAULT_KINDS)


def test_evaluator_runs_the_new_agents_on_the_device():
    """evaluate(batch, algorithms=[the three new names]): one row per (run, algorithm), each row the statistics of the facade agent's episode on
    that run alone (to 1e-9)."""
    from ev2gym_amd.baselines import heuristics as H
    from ev2gym_amd.env import EV2Gym
    from ev2gym_amd.evaluator import RESULT_STATS, evaluate
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(16, 10, 1, seed=9, power_setpoint_enabled=True))
    df = evaluate(batch, algorithms=list(NEW), seed=1)
    assert len(df) == 16 * len(NEW) and list(df["Algorithm"].unique()) == list(NEW)
    assert (df["time"] > 0).all()
    for name in NEW:
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


def test_new_device_agents_keep_the_rate_floor_at_cfg2():
    """Regression guard only: 4096 envs x 50 chargers, one whole episode per new agent through heuristic_run, at >= 20 M env-steps/s of
    kernel time (the floor tests/test_heuristics_gpu.py holds the first three agents to)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    batch = generate_native(GenConfig.v2g_profit_plus_loads(4096, 50, 1, seed=11, power_setpoint_enabled=True))
    eng = _engine(batch, DEFAULT_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    for name in NEW:
        a = eng.heuristic_create(name)
        for _ in range(2):   # warm-up episode, then the timed one
            eng.reset()
            eng.heuristic_run(a, T, None, 0, obs, 0, rew, 0, done, 0, mask, 0)
            rate = E * T / (eng.last_step_n_kernel_ms() / 1e3)
        eng.check_faults()
        print(name, f"{rate / 1e6:.1f} M env-steps/s")
        assert rate >= 20e6, (name, rate)
    eng.close()
