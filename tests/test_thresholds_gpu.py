"""Every step kernel against the CPU oracle with actions ON the reference's decision thresholds (tests/threshold_cases.py): exact ties of
`round(action, 5)` and of the efficiency table's key, amperes on the charger's `min - 0.01` edge and on the EV's minimum-power gate, charger
sums of exactly +-1 and one lattice step beyond, over-current steps.  A kernel whose last bit differs from the reference's at such a decision
(`rnd5_x`'s reciprocal division, a summation tree, an FMA) takes the other side: 1e-5 of an action, an efficiency step or a gated port -- the
suite's usual 1e-9 bar sees that, once the actions are there.  The oracle itself is held to the reference on such actions by the fixtures
tests/golden/edge_*.npz (tests/test_oracle_golden.py; the engine meets them in tests/test_engine_gpu.py).

Per kernel the route table can pick, at the smallest shape that reaches it, on a generated pool and on the crafted one (37 to 70 envs, whole
episodes, reward kinds 0, 1 and 4): single-step launches, one persistent launch, a persistent launch across an episode end, the float32 action
entry.  Observations, rewards and statistics to 1e-9 of max(1, |oracle|); masks, done, cycle counts and session ports exact; check_faults raises
exactly when the oracle reports over-current.  Every case asserts the floors of its classes (threshold_cases.FLOORS) before it compares anything.
The float32 entry (three cases per kernel and pool: `f32`, `f32_b`, `f32_c`) takes every policy; the oracle gets the float32 values widened.  The
three lattices are float32 values and keep their classes and floors.  `gate`'s five-decimal actions round back to themselves, so its edge and gate
classes, which are counted on the rounded action, stand too.  `dec` alone loses its class: the float32 nearest to (2k + 1) * 5e-6 is no tie any
more, it sits up to 6e-3 of a quantum beside one, so that case runs without a floor -- the one case here that asserts none.

`ev2g_step_big` has a test of its own with fewer modes: see its docstring."""
import numpy as np
import pytest

from tests import threshold_cases as tc

pytestmark = pytest.mark.gpu

_HET = dict(n_ports=np.array([3, 2, 2, 1, 1, 1]), transformer=np.array([0, 0, 0, 1, 1, 1]), min_charge_current=np.full(6, 6.0),
            max_charge_current=np.array([32.0, 16.0, 32.0, 16.0, 32.0, 16.0]), min_discharge_current=np.zeros(6),
            max_discharge_current=-np.array([32.0, 16.0, 32.0, 16.0, 32.0, 16.0]), voltage=np.array([230.0, 230.0, 400.0, 230.0, 400.0, 230.0]),
            phases=np.array([1, 1, 3, 1, 3, 1]), tr_max_power=np.array([60.0, 40.0]))
# id -> (generator arguments, EV2G_KERNEL, the kernel's name starts with, envs)
KERNELS = {
    "wave_p10": (dict(number_of_charging_stations=10), None, "ev2g_step_wave<", 70),                    # six envs per wavefront
    "wave_p50": (dict(number_of_charging_stations=50), None, "ev2g_step_wave<", 37),                    # one env per wavefront
    "v2_forced_p10": (dict(number_of_charging_stations=10), "v2", "ev2g_step_v2<256>", 70),
    "v2_forced_p50": (dict(number_of_charging_stations=50), "v2", "ev2g_step_v2<256>", 37),
    "v2_two_ports": (dict(number_of_charging_stations=12, number_of_ports_per_cs=2), None, "ev2g_step_v2<256>", 41),
    "v2_three_transformers": (dict(number_of_charging_stations=10, number_of_transformers=3, timescale=5, simulation_length=96, hour=8), None, "ev2g_step_v2<256>", 53),
    "generic_het": (dict(topology=_HET), None, "ev2g_step_kernel", 37),
}
# (pool kind, launch mode) -> the policy; the classes follow from the policy and the pool (classes_of)
POLICY = {("generated", "steps"): "lat64", ("generated", "persistent"): "latwild", ("generated", "across_end"): "dec",
          ("generated", "f32"): "lat64", ("generated", "f32_b"): "latwild", ("generated", "f32_c"): "dec",
          ("crafted", "steps"): "gate", ("crafted", "persistent"): "latwild", ("crafted", "across_end"): "lat32",
          ("crafted", "f32"): "gate", ("crafted", "f32_b"): "lat32", ("crafted", "f32_c"): "latwild"}
MODES = ("steps", "persistent", "across_end", "f32", "f32_b", "f32_c")   # the three f32 modes: one persistent launch each, through set_extras(actions_f32=...)
REWARDS = (0, 1, 4)   # ProfitMax_TrPenalty_UserIncentives, SquaredTrackingErrorReward, SquaredTrackingErrorRewardWithPenalty (its `usage == 0` test)
EXTRA_STEPS = 9       # of the second episode, in the launch across the episode end


def classes_of(pol, kind, pool, f32=False):
    multi = pool.ports_per_charger > 1
    if pol == "dec" and f32:   # no float32 value is a decimal tie
        return ()
    return {"lat64": ("round_ties",), "dec": ("round_ties",), "lat32": ("key_ties",) if kind == "crafted" else (),
            "gate": ("edge_near", "gate_near") if kind == "crafted" else (),
            "latwild": ("round_ties",) + (("sums",) if multi else ())}[pol]


_POOLS = {}


def pool_of(kernel, kind):
    from ev2gym_amd.scenario_gen import GenConfig, generate
    if (kernel, kind) not in _POOLS:
        kw, _, _, E = KERNELS[kernel]
        pool = generate(GenConfig(n_envs=E, spawn_multiplier=10.0, seed=40 + sorted(KERNELS).index(kernel), **kw))
        _POOLS[kernel, kind] = tc.craft(pool) if kind == "crafted" else pool
    return _POOLS[kernel, kind]


def _close(a, b, what, tol=1e-9):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), f"{what}: NaN pattern differs"
    err = np.nan_to_num(np.abs(a - b) / np.maximum(1.0, np.abs(np.nan_to_num(b))))
    assert err.max(initial=0.0) <= tol, f"{what}: max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def _state(eng, ora, envs, tag):
    """Port state that a flipped decision leaves behind: capacities, cycle counts (the sign test), sessions on the ports, the ports of the sessions."""
    for e in envs:
        pk, po = eng.peek(e), ora.peek(e)
        _close(pk["port_capacity"], po["cap"], f"{tag}: env {e} capacity")
        assert np.array_equal(pk["port_cycles"], po["cycles"]), f"{tag}: env {e} cycle counts"
        assert np.array_equal(pk["port_session"], po["session"]), f"{tag}: env {e} sessions on the ports"
        m = po["session_port"] >= 0
        assert np.array_equal(pk["session_port"][:len(m)][m], po["session_port"][m]), f"{tag}: env {e} session ports"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["generated", "crafted"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_step_kernel_on_the_decision_thresholds(kernel, kind, mode, monkeypatch):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine, EngineError
    from oracle.oracle import Oracle
    _, forced, name, E = KERNELS[kernel]
    if forced:
        monkeypatch.setenv("EV2G_KERNEL", forced)
    pool = pool_of(kernel, kind)
    case = (list(KERNELS).index(kernel) * 2 + (kind == "crafted")) * len(MODES) + MODES.index(mode)
    rk, sk = REWARDS[case % 3], (case // 3) % 3
    T, P = pool.n_steps, pool.n_ports
    K = T + EXTRA_STEPS if mode == "across_end" else T
    pol = POLICY[kind, mode]
    acts = tc.policy(pol, -1.0, (T, E, P), 100 + case, pool)
    if mode == "across_end":   # the same scenarios again (AUTO_RESET_SAME), other actions
        acts = np.concatenate([acts, tc.policy(pol, -1.0, (T, E, P), 900 + case, pool)[:EXTRA_STEPS]])
    tag = f"{kernel} {kind} {mode} {pol} rk={rk} sk={sk}"
    f32 = mode.startswith("f32")
    if f32:   # what the kernel reads; the counters and the oracle see the same values
        wide = acts.astype(np.float32).astype(np.float64)
        assert np.array_equal(wide, acts) == (pol in ("lat64", "lat32", "latwild")), "the lattices are float32 values, dec and gate are not"
    tc.assert_floors(tc.count_events((wide if f32 else acts)[:T], pool), classes_of(pol, kind, pool, f32), tag)
    if f32:
        assert pol == "dec" or np.array_equal(tc.rnd5(wide), tc.rnd5(acts)), "the float32 entry changes a rounded action"   # (dec: it does, to either side of the tie)
        acts = wide

    eng = Engine(pool, rk, sk, device=0, flags=4)
    assert eng.kernel_name.startswith(name), (eng.kernel_name, eng.fallback_reason)
    D = eng.D
    d_obs, d_rew, d_done, d_mask = eng.empty((K, E, D)), eng.empty((K, E)), eng.empty((K, E), np.uint8), eng.empty((K, E, P), np.uint8)
    if f32:
        d_act = None
        eng.set_extras(actions_f32=eng.empty((K, E, P), np.float32).upload(acts.astype(np.float32)))
    else:
        d_act = eng.empty((K, E, P)).upload(acts)
    ora = Oracle(pool, rk, sk)
    d_obs0 = eng.empty((E, D))
    eng.reset(d_obs0)
    _close(d_obs0.to_host(), ora.reset(), f"{tag}: reset obs")
    if mode == "steps":
        for t in range(T):
            eng.step(d_act.at(t * E * P), d_obs.at(t * E * D), d_rew.at(t * E), d_done.at(t * E), d_mask.at(t * E * P))
    else:
        eng.step_n(K, d_act, E * P, d_obs, E * D, d_rew, E, d_done, E, d_mask, E * P,
                   auto_reset=_abi.AUTO_RESET_SAME if mode == "across_end" else False, persistent=True)
    obs, rew, done, mask = d_obs.to_host(), d_rew.to_host(), d_done.to_host(), d_mask.to_host()
    faulted = first_faulted = False
    for k in range(K):
        if k == T:   # the episode end inside the launch: the first episode's statistics are gone, its rows were compared; the second starts
            first_faulted, faulted = faulted, False   # (the reset re-arms the env's fault flag: ev2g_check_faults reports the faults since the last reset)
            ora.close()
            ora = Oracle(pool, rk, sk)
            ora.reset()
        o, r, d, m, rc = ora.step(acts[k].copy())
        faulted = faulted or rc != 0
        assert np.array_equal(mask[k], m), f"{tag}: mask[{k}]"
        _close(obs[k], o, f"{tag}: obs[{k}]")
        _close(rew[k], r, f"{tag}: reward[{k}]")
        assert np.array_equal(done[k], d), f"{tag}: done[{k}]"
    _close(eng.stats(), ora.stats(), f"{tag}: statistics")
    _state(eng, ora, (0, E // 2, E - 1), tag)
    if faulted:
        with pytest.raises(EngineError, match="over-current"):
            eng.check_faults()
    else:   # also after a first episode that faulted: every reset, inside a launch too, clears the flag (the generic kernel's did not)
        eng.check_faults()
    eng.close()
    ora.close()


BIG_C, BIG_E, BIG_STEPS = 513, 5, 8   # ev2g_step_big's smallest shape in tests/test_round6_gpu.py, eight steps of it


@pytest.mark.parametrize("kind", ["generated", "crafted"])
def test_big_env_kernel_on_the_decision_thresholds(kind):
    """`ev2g_step_big` (specialisation 5): eight single-step launches from 08:00 on, where the EVs arrive, every output of every step; then the
    same eight steps as one launch.  The route (csrc/ev2g_route_host.h) gives a launch this kernel only for the default plugin pair (reward
    kind 0 on V2G_profit_max_loads), float64 actions, every output with step stride 0 and no auto-reset; anything else runs on
    ev2g_step_v2<1024>.  Hence reward kind 0 alone, no float32 entry and no launch across an episode end here, and of the one launch only the last
    step's outputs (stride 0 keeps no others) next to the port state all eight steps left behind; eight steps end no episode, so no statistics."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    from oracle.oracle import Oracle
    E, k = BIG_E, BIG_STEPS
    pool = generate_native(GenConfig.v2g_profit_plus_loads(E, BIG_C, 1, seed=613, hour=8, spawn_multiplier=10.0))
    pol = "lat64"
    if kind == "crafted":
        tc.craft(pool)
        pol = "gate"
    rk, sk = _abi.REWARD_KINDS["ProfitMax_TrPenalty_UserIncentives"], _abi.STATE_KINDS["V2G_profit_max_loads"]
    P = pool.n_ports
    acts = tc.policy(pol, -1.0, (k, E, P), 77, pool)
    tc.assert_floors(tc.count_events(acts, pool), classes_of(pol, kind, pool), f"ev2g_step_big {kind} {pol}")
    eng = Engine(pool, rk, sk, device=0, flags=_abi.FLAG_LOG_SOC)
    assert eng.big_kernel_reason == "", eng.big_kernel_reason
    ora = Oracle(pool, rk, sk)
    D = eng.D
    d_act = eng.empty((k, E, P)).upload(acts)
    obs, rew, done, mask = eng.empty((E, D)), eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.reset(obs)
    ora.reset()
    for t in range(k):
        eng.step_n(1, d_act.at(t * E * P), E * P, obs, 0, rew, 0, done, 0, mask, 0, auto_reset=False)
        assert eng.last_launch_specialisation == 5
        o, r, d, m, rc = ora.step(acts[t].copy())
        assert rc == 0
        assert np.array_equal(mask.to_host(), m), f"mask[{t}]"
        assert np.array_equal(done.to_host(), d), f"done[{t}]"
        _close(obs.to_host(), o, f"obs[{t}]")
        _close(rew.to_host(), r, f"reward[{t}]")
    _state(eng, ora, range(E), "single-step launches")
    eng.check_faults()
    eng.reset(obs)
    eng.step_n(k, d_act, E * P, obs, 0, rew, 0, done, 0, mask, 0, auto_reset=False, persistent=True)
    assert eng.last_launch_specialisation == 5
    assert np.array_equal(mask.to_host(), m) and np.array_equal(done.to_host(), d)
    _close(obs.to_host(), o, "last observation of the one launch")
    _close(rew.to_host(), r, "last reward of the one launch")
    _state(eng, ora, range(E), "one launch")
    eng.check_faults()
    ora.close()
    eng.close()
