"""The reference's action wrappers on the device (csrc/ev2g_wrap.h, ev2g_wrap_*; rl_agent/action_wrappers.py): the kernels against the
reference's own wrapper objects (the wrap_* fixtures) and against the numpy model of ev2gym_amd.rl_agent.action_wrappers (held to the reference
by tests/test_action_wrappers_cpu.py), bit for bit, through every layer above them."""
import os

import numpy as np
import pytest

from conftest import load_golden
from tests.test_action_wrappers_cpu import WRAP_DIR, WRAP_FIXTURES
from tests.test_heuristics_gpu import DEFAULT_KINDS, PST_KINDS, _engine

pytestmark = pytest.mark.gpu

REPAIR, BINARY, THREE = "Rescale_RepairLayer", "BinaryAction", "ThreeStep_Action"


def _model(eng, name, E=None):
    from ev2gym_amd.rl_agent.action_wrappers import WrapModel, charger_tables
    return WrapModel(name, eng.E if E is None else E, eng.P, *charger_tables(eng.batch.arrays))


def _state(eng):
    """What the repair layer reads of every env at the engine's current step, from ev2g_peek and the host's copies of the scenarios:
    connected, capacity, battery capacity, min / max AC charge power [E, P] and the step's setpoint [E]."""
    a, t = eng.batch.arrays, eng.current_step
    rows, sp = [], []
    n_sess = len(a["ev_B"])
    for e in range(eng.E):
        scn = (e + eng.scenario_offset) % eng.M
        pk = eng.peek(e)
        sess = pk["port_session"]
        conn = sess >= 0
        idx = np.minimum(a["env_session_start"][scn] + np.maximum(sess, 0), max(n_sess - 1, 0))
        pick = lambda k: np.where(conn, a[k][idx], 0.0) if n_sess else np.zeros(eng.P)   # noqa: E731
        rows.append((conn, np.where(conn, pk["port_capacity"], 0.0), np.where(conn, pick("ev_B"), 1.0), pick("ev_pac_min"), pick("ev_pac_max")))
        sp.append(a["power_setpoints"][scn, t])
    return tuple(np.array([r[i] for r in rows]) for i in range(5)) + (np.array(sp),)


def _model_action(eng, m, raw):
    return m.action(raw, *_state(eng)) if m.kind == 2 else m.action(raw)


def _lockstep(eng, w, m, raw, steps, f32=False, on_step=None):
    """steps x (ev2g_wrap_actions -> model on the same state -> ev2g_step on the device's wrapped actions): asserts bit equality at every
    step and returns the wrapped actions [steps, E, P]."""
    E, P = eng.E, eng.P
    a_in = eng.empty((E, P), np.float32 if f32 else np.float64)
    a_out = eng.empty((E, P))
    out = []
    for t in range(steps):
        a_in.upload(raw[t])
        want = _model_action(eng, m, np.float64(raw[t]))
        eng.wrap_actions(w, a_in, a_out, f32=f32)
        got = a_out.to_host()
        assert np.array_equal(got, want), (t, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
        if on_step:
            on_step(t)
        out.append(got.copy())
        eng.step(a_out)
    a_in.free()
    a_out.free()
    return np.array(out)


@pytest.mark.parametrize("name", WRAP_FIXTURES)
def test_wrap_run_reproduces_the_reference_wrappers_on_the_fixtures(name):
    """The raw actions the reference's wrapper object was given, through ev2g_wrap_run over the whole episode on three copies of the env: the
    wrapped rows are the reference's bit for bit and the step outputs match its trajectory (1e-9 relative, masks exactly)."""
    z, batch, rk, sk = load_golden(os.path.join(WRAP_DIR, name + ".npz"))
    eng = _engine(batch.tile(3), (str(z["case"][3]), str(z["case"][2])))
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    w = eng.wrap_create(str(z["wrap_class"]))
    raw = eng.empty((T, E, P)).upload(np.tile(z["wrap_raw"][:, None, :], (1, E, 1)))
    wrapped, obs, rew = eng.empty((T, E, P)), eng.empty((T, E, D)), eng.empty((T, E))
    done, mask = eng.empty((T, E), np.uint8), eng.empty((T, E, P), np.uint8)
    eng.reset()
    eng.wrap_run(w, T, raw, E * P, wrapped, E * P, obs, E * D, rew, E, done, E, mask, E * P)
    assert eng.last_step_n_kernel_ms() > 0
    got, o, r, mk, dn = wrapped.to_host(), obs.to_host(), rew.to_host(), mask.to_host(), done.to_host()
    eng.check_faults()
    eng.close()
    assert dn[-1].all() and not dn[:-1].any()
    for t in range(T):
        for e in range(E):
            assert np.array_equal(got[t, e], z["wrap_act"][t]), (name, t, e, got[t, e], z["wrap_act"][t])
            ref = z["trj_obs"][t + 1]
            assert (np.abs(o[t, e] - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-9, (name, t, e)
            assert abs(r[t, e] - z["trj_reward"][t]) <= 1e-9 * max(1.0, abs(z["trj_reward"][t])), (name, t, e)
            assert (mk[t, e] == z["trj_mask"][t]).all(), (name, t, e)


# setpoint of a step as a share of (ports occupied at that step x the charger's power): 0 and 0.15 lie below what the queued EVs draw at their
# minimum powers (0.25 of a charger each at 4 A of 16 A: a full reduction), 0.3 .. 0.4 between that and what rescaled uniform actions ask for
# (about 0.5: a partial reduction, whose rounding the greedy top-up repairs about every other time), 1 and 2 above it (a raise)
SETPOINT_SHARES = (0.0, 0.15, 0.3, 0.35, 0.4, 1.0, 2.0)


def occupied_ports(batch):
    """[E, T]: the ports whose session window covers the step, from the scenario arrays."""
    from ev2gym_amd.scenario import resolve_ports
    a, port = batch.arrays, resolve_ports(batch)
    E, P, T = batch.n_envs, batch.n_ports, batch.n_steps
    occ = np.zeros((E, P, T), bool)
    for e in range(E):
        for s in range(int(a["env_session_start"][e]), int(a["env_session_start"][e + 1])):
            if port[s] >= 0:
                occ[e, port[s], max(int(a["ev_t_arr"][s]), 0):min(int(a["ev_t_dep"][s]), T - 1) + 1] = True
    return occ.sum(1)


def repair_batch(P, E=5, seed=None, unequal=False, min_current=4.0):
    """The generator's PublicPST kind at P one-port chargers, 32 steps from 9 o'clock with many arrivals, non-zero minimum powers, and setpoints
    redrawn as SETPOINT_SHARES of the occupied ports' charger power, so that the queued power lies above and below them.  At 4 A the chargers'
    minimum power (2.8 kW) is below every EV's maximum; at 6 A (4.2 kW) the 3.6 / 3.7 kW EVs enter the queue with min_power > max_power, and a
    reduction then lifts them to min_power: its total never ends below the setpoint and no top-up follows."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    seed = 30 + P if seed is None else seed
    batch = generate(GenConfig.public_pst(E, P, seed=seed, hour=9, spawn_multiplier=40, cs_min_charge_current=min_current, simulation_length=32))
    rng = np.random.default_rng(seed)
    a = batch.arrays
    kw = a["cs_max_charge_current"][0] * a["cs_voltage"][0] * np.sqrt(float(a["cs_phases"][0])) / 1000
    a["power_setpoints"][:] = occupied_ports(batch) * kw * rng.choice(SETPOINT_SHARES, a["power_setpoints"].shape)
    if unequal:
        a["cs_max_charge_current"][::2] = 32.0
    return batch


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_randomised_repair_layer_equals_the_model(P):
    """5 envs (not a multiple of the wavefronts per workgroup), port counts around one and two 64-entry chunks of the queue: the device's
    wrapped actions are the model's at every step, and every branch occurs."""
    from ev2gym_amd.rl_agent import action_wrappers as AW
    batch = repair_batch(P)
    assert batch.n_envs == 5 and batch.n_ports == P == batch.n_chargers and batch.n_steps == 32
    eng = _engine(batch, PST_KINDS)
    w, m = eng.wrap_create(REPAIR), _model(eng, REPAIR)
    counts, longest = np.zeros(5, np.int64), [0]

    def seen(t):
        counts[:] += np.bincount(m.branch, minlength=5)
        longest[0] = max(longest[0], int(m.qlen.max()))

    raw = np.random.default_rng(P).uniform(0, 1, (eng.T, eng.E, P))
    eng.reset()
    out = _lockstep(eng, w, m, raw, eng.T, on_step=seen)
    eng.check_faults()
    eng.close()
    print(f"P={P}: branches pass/raise/raise-no-range/reduce/top-up {counts.tolist()}, longest queue {longest[0]}")
    assert (out != 0).any()
    # every branch: the setpoint shares put about a third of the steps into each of raise / full reduction / partial reduction, the first steps
    # of every env have no EV yet (pass under a zero setpoint, a raise without range under a positive one)
    assert counts[AW.RAISE] >= 3 and counts[AW.REDUCE] >= 3 and counts[AW.REDUCE_TOPUP] >= 1 and counts[AW.PASS] + counts[AW.RAISE_NO_RANGE] >= 1, counts
    if P == 130:
        assert longest[0] >= 70, longest   # the queue crosses a 64-entry chunk


def test_float32_input_equals_float64_input_on_the_widened_values():
    batch = repair_batch(20, seed=7)
    eng = _engine(batch, PST_KINDS)
    E, P = eng.E, eng.P
    raw32 = np.random.default_rng(3).uniform(0, 1, (12, E, P)).astype(np.float32)
    raw32[:, :, 0], raw32[:, :, 1] = 0.0, 1.0
    for name in (REPAIR, BINARY, THREE):
        w32, w64 = eng.wrap_create(name), eng.wrap_create(name)
        a32, a64, o32, o64 = eng.empty((E, P), np.float32), eng.empty((E, P)), eng.empty((E, P)), eng.empty((E, P))
        eng.reset()
        for t in range(12):
            a32.upload(raw32[t])
            a64.upload(np.float64(raw32[t]))
            eng.wrap_actions(w32, a32, o32, f32=True)
            eng.wrap_actions(w64, a64, o64)
            got = o32.to_host()
            assert np.array_equal(got, o64.to_host()), (name, t)
            eng.step(o64)
        assert (got != np.float64(raw32[-1])).any()
    eng.close()


def test_wrap_actions_in_place():
    """`out` aliasing a float64 `in`: the block is rewritten in place, for every kind."""
    batch = repair_batch(65, seed=8, min_current=6.0)   # (with min_power > max_power entries)
    eng = _engine(batch, PST_KINDS)
    E, P = eng.E, eng.P
    raw = np.random.default_rng(4).uniform(0, 1, (10, E, P))
    raw[:, :, :3] = (0.0, 1.0, 2.0)
    for name in (REPAIR, BINARY, THREE):
        w, m = eng.wrap_create(name), _model(eng, name)
        buf = eng.empty((E, P))
        eng.reset()
        for t in range(10):
            buf.upload(raw[t])
            want = _model_action(eng, m, raw[t])
            eng.wrap_actions(w, buf, buf)
            assert np.array_equal(buf.to_host(), want), (name, t)
            eng.step(buf)
    eng.close()


def test_the_queue_survives_a_reset_is_emptied_on_request_and_belongs_to_its_wrapper():
    """Chargers of unequal power (the queue's order and the powers kept with its entries show in the actions).  Wrapper A runs half an
    episode; wrapper B, created then, starts empty: on the same states each equals its own model and the two differ.  ev2g_reset leaves A's
    queue alone: after a reset in mid-episode, with entries queued, A goes on equal to the model that was not reset (no port holds an EV
    at step 0 -- the engine's sessions arrive at step 1 or later -- so the entries carried over a reset are dropped by the first update, in
    the model as on the device).  ev2g_wrap_reset_state in mid-episode makes A a fresh wrapper: it equals the emptied model and differs from
    a copy that kept the queue."""
    import copy
    batch = repair_batch(12, E=4, seed=21, unequal=True)
    eng = _engine(batch, PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    raw = np.random.default_rng(5).uniform(0, 1, (3 * T, E, P))
    a, kept = eng.wrap_create(REPAIR), _model(eng, REPAIR)
    a_in, out_a, out_b = eng.empty((E, P)), eng.empty((E, P)), eng.empty((E, P))

    def both(other, model, t, r):
        """A and `other` (a device wrapper, or None) on the same state against `kept` and `model`; steps with A's actions; 1 if the two differ"""
        a_in.upload(r)
        st = _state(eng)
        want_a, want_b = kept.action(r, *st), model.action(r, *st)
        eng.wrap_actions(a, a_in, out_a)
        assert np.array_equal(out_a.to_host(), want_a), t
        if other is not None:
            eng.wrap_actions(other, a_in, out_b)
            assert np.array_equal(out_b.to_host(), want_b), t
        eng.step(out_a)
        return int(not np.array_equal(want_a, want_b))

    eng.reset()
    _lockstep(eng, a, kept, raw, T // 2)
    assert kept.qlen.max() >= 2, kept.qlen   # something that a fresh wrapper lacks
    b, fresh = eng.wrap_create(REPAIR), _model(eng, REPAIR)
    differ = sum(both(b, fresh, t, raw[t]) for t in range(T // 2, 3 * T // 4))
    assert differ > 0, "two wrappers of one handle must not share a queue"
    assert kept.qlen.max() >= 2, kept.qlen   # carried into the reset
    eng.reset()
    _lockstep(eng, a, kept, raw[T:], T // 2)
    stale = copy.deepcopy(kept)
    eng.wrap_reset_state(a)
    kept.reset_state()
    differ = sum(both(None, stale, t, raw[T + t]) for t in range(T // 2, T))
    assert differ > 0, "emptying the queue must show in the actions"
    eng.check_faults()
    eng.close()


@pytest.mark.parametrize("name", [REPAIR, BINARY])
def test_wrap_rollout_equals_the_hand_made_chain(name):
    """ev2g_wrap_rollout against ev2g_mlp_forward -> ev2g_wrap_actions(float32 in) -> ev2g_step between the registered float32 buffers, bit
    for bit, on a V2GProfitPlusLoads shape with the actor's outputs in (0, 1)."""
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(8, 10, 1, seed=17, power_setpoint_enabled=True, hour=9, spawn_multiplier=20, simulation_length=32))
    eng = _engine(batch, DEFAULT_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9, h1=32, h2=32), out_lo=0.0)
    obs32, act32 = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
    eng.set_extras(obs_f32=obs32, actions_f32=act32)
    k = 24
    rew, done, mask = eng.empty((k, E)), eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)
    w = eng.wrap_create(name)
    eng.reset_f32(obs32, 0)
    eng.wrap_rollout(w, mlp, k, rew, E, done, E, mask, E * P)
    assert eng.current_step == k and eng.last_step_n_kernel_ms() > 0
    got = dict(rew=rew.to_host(), done=done.to_host(), mask=mask.to_host(), obs=obs32.to_host(), act=act32.to_host())
    w2 = eng.wrap_create(name)
    wrapped, r1, d1, m1 = eng.empty((E, P)), eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.reset_f32(obs32, 0)
    changed = 0
    for t in range(k):
        eng.mlp_forward(mlp, obs32, act32, E)
        eng.wrap_actions(w2, act32, wrapped, f32=True)
        changed += int((wrapped.to_host() != np.float64(act32.to_host())).sum())
        eng.step(wrapped, None, r1, d1, m1)
        assert np.array_equal(got["rew"][t], r1.to_host()) and np.array_equal(got["mask"][t], m1.to_host()), (name, t)
    assert np.array_equal(got["obs"], obs32.to_host()) and np.array_equal(got["act"], act32.to_host()) and changed > 0
    assert np.abs(got["rew"]).sum() > 0
    eng.set_extras()
    eng.close()


@pytest.mark.parametrize("npc", [2, 3])
def test_discretisers_on_multi_port_chargers(npc):
    """BinaryAction and ThreeStep_Action with 2 and 3 ports per charger and chargers of unequal minimum current: min_action is the port's
    charger's; the 0.5 and 0 / 1 boundaries are hit exactly."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(5, 7, 1, seed=12 + npc, number_of_ports_per_cs=npc, cs_min_charge_current=6.0))
    batch.arrays["cs_min_charge_current"][::2] = 10.0
    eng = _engine(batch, DEFAULT_KINDS)
    E, P = eng.E, eng.P
    assert P == 7 * npc
    rng = np.random.default_rng(npc)
    for name in (BINARY, THREE):
        w, m = eng.wrap_create(name), _model(eng, name)
        assert len(np.unique(m.min_action)) == 2 and (m.min_action.reshape(7, npc) == m.min_action.reshape(7, npc)[:, :1]).all()
        raw = rng.choice([0.0, 0.5, 1.0, 2.0, -1.0, 0.25, 0.75, np.nextafter(0.5, 1)], (4, E, P))
        eng.reset()
        out = _lockstep(eng, w, m, raw, 4)
        assert set(np.unique(out)) <= {0.0, 1.0, *m.min_action}
    eng.close()


def test_refusals():
    """Code and message of every refusal; nothing is launched and the step counter stays."""
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate

    def refused(call, code, words):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == code and words in str(ei.value), (code, words, str(ei.value))

    one = generate(GenConfig.v2g_profit_plus_loads(4, 10, 1, seed=13, power_setpoint_enabled=True, simulation_length=16))
    two = generate(GenConfig.v2g_profit_plus_loads(4, 5, 1, seed=14, number_of_ports_per_cs=2, power_setpoint_enabled=True, simulation_length=16))
    eng, other = _engine(one, DEFAULT_KINDS), _engine(one, DEFAULT_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    act, out = eng.empty((E, P)).upload(np.full((E, P), 0.5)), eng.empty((E, P))
    for kind in (3, -1):
        refused(lambda: eng.wrap_create(kind), -1, "unknown wrapper kind")
    w, far = eng.wrap_create(REPAIR), other.wrap_create(REPAIR)
    three = eng.wrap_create(THREE)
    eng.reset()
    # a foreign and a destroyed object
    gone = eng.wrap_create(BINARY)
    eng.wrap_destroy(gone)
    for x in (far, gone):
        refused(lambda: eng.wrap_actions(x, act, out), -1, "the wrapper was not created on this handle")
        refused(lambda: eng.wrap_run(x, 1, act), -1, "the wrapper was not created on this handle")
        refused(lambda: eng.wrap_reset_state(x), -1, "the wrapper was not created on this handle")
    # null actions, a segment past the episode end
    refused(lambda: eng.wrap_run(w, 1, None), -1, "actions")
    refused(lambda: eng.wrap_actions(w, None, out), -1, "null")
    refused(lambda: eng.wrap_run(w, T + 1, act), -4, "the segment would run past the episode end")
    assert eng.current_step == 0
    # ThreeStep_Action in a rollout; a rollout without the registered pair
    mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9, h1=32, h2=32), out_lo=0.0)
    refused(lambda: eng.wrap_rollout(w, mlp, 1), -1, "register float32 observation")
    obs32, act32 = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
    eng.set_extras(obs_f32=obs32, actions_f32=act32)
    refused(lambda: eng.wrap_rollout(three, mlp, 1), -1, "ThreeStep_Action")
    eng.set_extras()
    eng.wrap_run(w, T, act)
    refused(lambda: eng.wrap_actions(w, act, out), -4, "episode is done")
    refused(lambda: eng.wrap_run(w, 1, act), -4, "past the episode end")
    # a reload to two-port chargers under a live repair layer (same envs and ports): refused from then on, the discretiser goes on
    eng.load(two)
    eng.reset()
    refused(lambda: eng.wrap_actions(w, act, out), -1, "one port per charger")
    refused(lambda: eng.wrap_run(w, 1, act), -1, "one port per charger")
    refused(lambda: eng.wrap_create(REPAIR), -1, "one port per charger")
    eng.wrap_actions(three, act, out)
    assert eng.current_step == 0
    # other envs / ports under a live wrapper
    eng.load(generate(GenConfig.v2g_profit_plus_loads(4, 6, 1, seed=15, simulation_length=16)))
    refused(lambda: eng.wrap_actions(three, act, out), -1, "envs / ports differ")
    eng.close()
    other.close()
    # above the port limit
    big = generate(GenConfig.public_pst(1, 2260, seed=1, simulation_length=4))
    eng = _engine(big, PST_KINDS)
    refused(lambda: eng.wrap_create(REPAIR), -1, "up to 2259 ports")
    eng.wrap_create(BINARY)
    eng.close()


@pytest.mark.parametrize("name", ["wrap_repair_pst_unequal_s5", "wrap_repair_v2gppl_sp_s5"])
def test_python_wrappers_reproduce_a_repair_fixture(name):
    """Rescale_RepairLayer around an EV2GymVec and around the single-env facade, driven with the fixture's raw actions: the reference's
    wrapped actions bit for bit, its observations and rewards to 1e-9."""
    from ev2gym_amd.env import EV2Gym
    from ev2gym_amd.rl_agent.action_wrappers import Rescale_RepairLayer
    from ev2gym_amd.vec_env import EV2GymVec
    z, batch, rk, sk = load_golden(os.path.join(WRAP_DIR, name + ".npz"))
    kinds = dict(state_function=str(z["case"][2]), reward_function=str(z["case"][3]))
    T = len(z["wrap_raw"])

    def close_to(got, ref):
        return (np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-9

    vec = Rescale_RepairLayer(EV2GymVec(scenarios=batch, num_envs=1, auto_reset=False, use_torch=False, **kinds))
    vec.reset()
    for t in range(T):
        obs, rew, done, _, info = vec.step(z["wrap_raw"][t][None])
        assert np.array_equal(vec.unwrapped._act.to_host()[0], z["wrap_act"][t]), (name, t)
        assert close_to(obs[0], z["trj_obs"][t + 1]) and close_to(rew[0], z["trj_reward"][t]), (name, t)
    assert done.all()
    vec.close()
    env = Rescale_RepairLayer(EV2Gym(scenario=batch, **kinds))
    env.reset()
    for t in range(T):
        want = env.action(z["wrap_raw"][t])
        assert np.array_equal(want, z["wrap_act"][t]), (name, t)
        # (action() updated the queue as the reference's does; the step below repeats it on the same state, which changes nothing)
        obs, rew, done, _, info = env.step(z["wrap_raw"][t])
        assert close_to(obs, z["trj_obs"][t + 1]) and close_to(rew, z["trj_reward"][t]), (name, t)
    assert done
    env.close()


def test_python_wrapper_carries_its_queue_over_an_auto_reset():
    """EV2GymVec(auto_reset=True) under ONE Rescale_RepairLayer across an episode end: the second episode's wrapped actions are those of the
    model that was never reset.  (The generator leaves every port empty at the end of an episode, as the reference's spawner does, so the
    queue carried over a natural episode end is empty; entries carried over a reset are in the mid-episode reset of the test above.)"""
    from ev2gym_amd.rl_agent.action_wrappers import Rescale_RepairLayer
    from ev2gym_amd.vec_env import EV2GymVec
    E = 4
    pool = repair_batch(12, E=2 * E, seed=22, unequal=True)
    vec = EV2GymVec(scenarios=pool, num_envs=E, state_function=PST_KINDS[1], reward_function=PST_KINDS[0], auto_reset=True, use_torch=False, seed=3)
    w = Rescale_RepairLayer(vec)
    eng = vec.engine
    m = _model(eng, "Rescale_RepairLayer")
    raw = np.random.default_rng(6).uniform(0, 1, (eng.T + 10, E, eng.P))
    w.reset()
    for t in range(eng.T + 10):
        if t == eng.T:
            assert eng.current_step == 0   # the env has reset itself; nobody has reset the wrapper
        want = m.action(raw[t], *_state(eng))
        w.step(raw[t])
        assert np.array_equal(vec._act.to_host(), want), t
    w.close()
