"""ev2g_load_scenarios seen through the C-ABI: every refusal's code and full message, which of two faults is reported, what a refusal
leaves of the pool that was loaded before, the kernel routing under each environment switch, and that loads do not leak into each other.
Everything here holds for the loader as one function and as the host-only plan (csrc/ev2g_load_host.h) plus the device stage.

Shapes: hand-built batches of 2 scenarios x 2 single-port chargers x 16 steps with two sessions each (the faults are one changed number
of that batch); routing on 1, 2, 4, 64, 65 ports and two handles of 513 and 1024 ports (2 scenarios, 8 steps) for ev2g_step_big.

A refusal of the shape checks at the front leaves the loaded pool loaded and usable; any later one leaves the handle unloaded."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
PRE = "ev2g_load_scenarios: "


def hand_batch(chargers=((0, 1, 3), (0, 1, 3)), sessions=(((0, 2, 5), (1, 3, 6)), ((1, 1, 4), (0, 4, 9))), T=16, R=1, seed=0):
    """chargers: (transformer, ports, phases) each; sessions: per scenario (charger, t_arr, t_dep) in arrival order."""
    from ev2gym_amd.scenario import ScenarioBatch
    M, Cn = len(sessions), len(chargers)
    rng = np.random.default_rng(seed)
    flat = [s for ss in sessions for s in ss]
    S = len(flat)
    ph = np.array([c[2] for c in chargers], np.int32)
    B = rng.choice([40.0, 60.0], S)
    a = dict(
        cs_min_charge_current=np.full(Cn, 6.0), cs_max_charge_current=np.full(Cn, 32.0), cs_min_discharge_current=np.full(Cn, -6.0),
        cs_max_discharge_current=np.full(Cn, -32.0), cs_voltage=np.where(ph == 3, 400.0, 230.0), cs_phases=ph,
        cs_transformer=np.array([c[0] for c in chargers], np.int32), cs_n_ports=np.array([c[1] for c in chargers], np.int32),
        charge_price=-rng.uniform(0.05, 0.3, (M, T)), discharge_price=rng.uniform(0.05, 0.3, (M, T)), power_setpoints=rng.uniform(5.0, 40.0, (M, T)),
        tr_max_power=np.full((M, R, T), 400.0), tr_min_power=np.full((M, R, T), -400.0), tr_inflexible_load=rng.uniform(5.0, 20.0, (M, R, T)),
        tr_solar_power=-rng.uniform(0.0, 5.0, (M, R, T)), tr_dr=np.zeros((M, R, 1, 3)), tr_n_dr=np.zeros((M, R), np.int32), tr_steps_ahead=np.full((M, R), 4, np.int32),
        env_session_start=np.cumsum([0] + [len(ss) for ss in sessions]).astype(np.int64),
        ev_cs=np.array([s[0] for s in flat], np.int32), ev_t_arr=np.array([s[1] for s in flat], np.int32), ev_t_dep=np.array([s[2] for s in flat], np.int32),
        ev_phases=np.array([1 + i % 3 for i in range(S)], np.int32), ev_lut=np.full(S, -1, np.int32),
        ev_cap0=0.3 * B, ev_B=B, ev_desired=0.9 * B, ev_minB=0.1 * B, ev_min_emerg=0.2 * B, ev_pac_max=rng.choice([7.4, 11.0], S), ev_pac_min=np.zeros(S),
        ev_pdis_max=np.full(S, -7.0), ev_pdis_min=np.zeros(S), ev_ts=np.full(S, 0.8), ev_tsm=np.full(S, 0.5), ev_eta_ch=np.full(S, 0.93),
        ev_eta_dis=np.full(S, 0.91), lut=np.zeros((0, 101)))
    a["tr_load_forecast"], a["tr_pv_forecast"] = a["tr_inflexible_load"].copy(), a["tr_solar_power"].copy()
    return ScenarioBatch(M, T, 15, Cn, max(c[1] for c in chargers), R, arrays=a).finalize()


def spread(n_ports, n_sessions=6, T=8, M=2):
    """`n_ports` single-port chargers on one transformer, one session each on a few of the first and the last chargers."""
    n = min(n_sessions, n_ports)
    ss = tuple((n_ports - 1 - i // 2 if i % 2 else i // 2, 1 + (4 * i) // n, 2 + (4 * i) // n + i % 3) for i in range(n))
    return hand_batch(chargers=((0, 1, 3),) * n_ports, sessions=(ss,) * M, T=T)


def engine(batch, state="V2G_profit_max", reward="ProfitMax_TrPenalty_UserIncentives", flags=None, **kw):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    return Engine(batch, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], device=0, flags=_abi.FLAG_LOG_SOC if flags is None else flags, **kw)


def episode(eng, k=None, seed=7):
    """obs [k+1,E,D] and reward [k,E] of k steps from a reset under a fixed uniform action block, one-step launches."""
    E, P, D = eng.E, eng.P, eng.D
    k = k or eng.T
    acts, obs, rew, done, mask = eng.empty((k, E, P)), eng.empty((E, D)), eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.fill_uniform(acts, k * E * P, seed, -1.0, 1.0)
    eng.reset(obs)
    o, r = [obs.to_host().copy()], []
    for t in range(k):
        eng.step(acts.at(t * E * P), obs, rew, done, mask)
        o.append(obs.to_host().copy()), r.append(rew.to_host().copy())
    for b in (acts, obs, rew, done, mask):
        b.free()
    return np.array(o), np.array(r)


def launch(eng, k=2, strided=False):
    """One persistent launch of k steps with every output present: step stride 0, or [k, E, *] blocks."""
    E, P, D = eng.E, eng.P, eng.D
    n = k if strided else 1
    acts, obs, rew, done, mask = eng.empty((k, E, P)), eng.empty((n, E, D)), eng.empty((n, E)), eng.empty((n, E), np.uint8), eng.empty((n, E, P), np.uint8)
    eng.fill_uniform(acts, k * E * P, 3, 0.0, 1.0)
    eng.reset()
    st = (E * D, E, E, E * P) if strided else (0, 0, 0, 0)
    eng.step_n(k, acts, E * P, obs, st[0], rew, st[1], done, st[2], mask, st[3], auto_reset=False, persistent=True)
    eng.synchronize()
    return eng.last_launch_specialisation


# ---- the faults, in the order the loader checks them: (id, fault(cb, arrays), message) -------------------------------------------------------
def _set(name, i, v):
    return lambda cb, a: a[name].__setitem__(i, v)


def _field(**kw):
    return lambda cb, a: [setattr(cb, k, v) for k, v in kw.items()]


def _both(*fs):
    return lambda cb, a: [f(cb, a) for f in fs]


def _many_sessions(cb, a):
    a["env_session_start"][-1] = 0x7ffffff1
    cb.n_sessions = 0x7ffffff1


def _rising(cb, a):   # port counts 1, 2: the reference's mask index of charger 1 leaves the 3-entry array
    a["cs_n_ports"][:] = [1, 2]
    cb.ports_per_charger = max(cb.ports_per_charger, 2)


M16 = (PRE + "simulation_length and the number of efficiency tables must stay below 65536 (a port's state line packs charging_cycles and the "
       "table id into 16 bits each)")
NO_PORT = PRE + "no free port for a session (assert n_evs_connected < n_ports, ev_charger.py:271)"
FRONT = [   # the shape checks: the pool loaded before stays
    ("n_active_envs", _field(n_envs=1), PRE + "n_active_envs exceeds the number of scenarios in the batch"),
    ("non_positive", _field(n_steps=0), PRE + "non-positive size"),
    ("horizon", _field(horizon=10), PRE + "horizon must be 20 (state.py:119,129-132)"),
    ("ports_per_charger_33", _field(ports_per_charger=33), PRE + "more than 32 ports per charger unsupported"),
    ("cs_n_ports_0", _set("cs_n_ports", 1, 0), PRE + "cs_n_ports must be >= 1"),
    ("ports_per_charger_not_max", _field(ports_per_charger=3), PRE + "ports_per_charger must be the maximum of cs_n_ports"),
    ("action_mask", _rising, PRE + "this charger order makes the reference's action mask index i*n_ports+j leave the mask array (ev2gym_env.py:457 "
                                   "raises IndexError); order the chargers by falling port count"),
    ("n_sessions", lambda cb, a: setattr(cb, "n_sessions", cb.n_sessions + 1), PRE + "env_session_start inconsistent with n_sessions"),
    ("too_many_sessions", _many_sessions, PRE + "too many sessions for 32-bit indices"),
    ("element_offsets", _field(n_steps=65535, n_transformers=16500), PRE + "batch too large for 32-bit element offsets (need M*P, M*D, M*R*(T+1)*40, "
                                                                           "T*M*C < 2^31): split it over more handles / GPUs"),
    ("n_lut", _field(n_lut=65535), M16),
    ("cs_transformer", _set("cs_transformer", 0, 1), PRE + "cs_transformer out of range"),
    ("cs_phases", _set("cs_phases", 0, 4), PRE + "cs_phases must be 1..3"),
]
LATE = [    # from the session replay on: the handle is left unloaded
    ("not_monotone", _set("env_session_start", 1, -1), PRE + "env_session_start not monotone"),
    ("ev_cs", _set("ev_cs", 0, 7), PRE + "ev_cs out of range"),
    ("t_arr", _set("ev_t_arr", 0, 0), PRE + "need 1 <= t_arr <= t_dep"),
    ("unsorted", _set("ev_t_arr", 1, 1), PRE + "sessions must be sorted by arrival"),
    ("ev_phases", _set("ev_phases", 1, 0), PRE + "ev_phases must be 1..3"),
    ("ev_lut", _set("ev_lut", 1, 0), PRE + "ev_lut out of range"),
    ("no_free_port", _set("ev_cs", 1, 0), NO_PORT),
]
EXTRA = [   # the other halves of checks with two conditions
    ("first_session_start", "front", _set("env_session_start", 0, 1), PRE + "env_session_start inconsistent with n_sessions"),
    ("simulation_length", "front", _field(n_steps=65536), M16),
    ("cs_transformer_negative", "front", _set("cs_transformer", 1, -1), PRE + "cs_transformer out of range"),
    ("t_dep_before_t_arr", "late", _set("ev_t_dep", 1, 2), PRE + "need 1 <= t_arr <= t_dep"),
    ("ev_cs_negative", "late", _set("ev_cs", 1, -1), PRE + "ev_cs out of range"),
]
# one input with the faults of two adjacent checks: the earlier check reports.  (t_arr = 0 at the second session is below 1 AND below the first
# arrival; the three-number element_offsets fault keeps its n_steps when n_lut joins it.)
CHECKS = FRONT + LATE
PAIRS = [(CHECKS[i][0] + "+" + CHECKS[i + 1][0], "front" if i < len(FRONT) else "late", _both(CHECKS[i + 1][1], CHECKS[i][1]), CHECKS[i][2])
         for i in range(len(CHECKS) - 1) if CHECKS[i][0] != "t_arr"]
PAIRS.append(("t_arr+unsorted", "late", _set("ev_t_arr", 1, 0), PRE + "need 1 <= t_arr <= t_dep"))
CASES = [(n, "front", f, m) for n, f, m in FRONT] + [(n, "late", f, m) for n, f, m in LATE] + EXTRA + PAIRS


class Loaded:
    """A handle for two envs with the hand batch loaded, its reference trajectory and an action block to step it with."""

    def __init__(self, **kw):
        self.base = hand_batch()
        self.eng = engine(self.base, n_active_envs=2, **kw)
        self.want = episode(self.eng, 6)
        self.acts = self.eng.empty((2, 2))
        self.eng.fill_uniform(self.acts, 4, 1, -1.0, 1.0)

    def refuse(self, fault, message, stage, reload=True):
        eng, lib = self.eng, self.eng._lib
        batch = hand_batch()
        cb = batch.to_c()
        fault(cb, batch.arrays)
        rc = lib.ev2g_load_scenarios(eng._h, C.byref(cb))
        assert (rc, eng.last_error()) == (ARG, message)
        if stage == "front":   # the old pool is still there: same kernel, same trajectory
            assert eng.kernel_name.startswith("ev2g_step_wave")
            got = episode(eng, 6)
            np.testing.assert_array_equal(got[0], self.want[0]), np.testing.assert_array_equal(got[1], self.want[1])
        else:
            assert lib.ev2g_step(eng._h, self.acts.ptr, None, None, None, None) == STATE
            assert eng.last_error() == "ev2g_step: no scenarios loaded" and eng.kernel_name == ""
            assert lib.ev2g_reset(eng._h, None) == STATE
            if not reload:
                return
            eng.load(self.base)
            got = episode(eng, 6)
            np.testing.assert_array_equal(got[0], self.want[0]), np.testing.assert_array_equal(got[1], self.want[1])


@pytest.fixture(scope="module")
def loaded():
    x = Loaded()
    yield x
    x.eng.close()


@pytest.mark.parametrize("name,stage,fault,message", CASES, ids=[c[0] for c in CASES])
def test_refusal_code_message_and_what_is_left_of_the_old_pool(loaded, name, stage, fault, message):
    loaded.refuse(fault, message, stage)


def test_null_arguments(loaded):
    lib, eng = loaded.eng._lib, loaded.eng
    assert lib.ev2g_load_scenarios(eng._h, None) == ARG and eng.last_error() == PRE + "null argument"
    cb = loaded.base.to_c()
    assert lib.ev2g_load_scenarios(None, C.byref(cb)) == ARG and (lib.ev2g_last_error(None) or b"").decode() == PRE + "null argument"
    assert eng.kernel_name.startswith("ev2g_step_wave")   # (still loaded)


def test_refillable_session_slots_and_the_lds_capacity(monkeypatch):
    """The two refusals that need their own handle: the session slots of a refillable pool (between the shape checks and the session
    replay), and an env whose ports do not fit the LDS staging (after the replay: a session without a free port is reported first)."""
    from ev2gym_amd import _abi
    x = Loaded(flags=_abi.FLAG_LOG_SOC | _abi.FLAG_REFILLABLE)
    try:
        assert x.eng.pool_session_capacity == 16   # ((2 + 2 // 4 + 8) + 7) // 8 * 8
        monkeypatch.setenv("EV2G_POOL_SESSION_CAP", str(1 << 30))
        slots = PRE + "too many session slots for 32-bit indices (refillable pool)"
        x.refuse(_set("cs_phases", 0, 4), PRE + "cs_phases must be 1..3", "front")
        x.refuse(lambda cb, a: None, slots, "late", reload=False)
        x.refuse(_set("env_session_start", 1, -1), slots, "late", reload=False)
        monkeypatch.setenv("EV2G_POOL_SESSION_CAP", "96")
        x.eng.load(x.base)
        assert x.eng.pool_session_capacity == 96
        monkeypatch.delenv("EV2G_POOL_SESSION_CAP")
        x.eng.load(x.base)
        assert x.eng.pool_session_capacity == 16
        got = episode(x.eng, 6)
        np.testing.assert_array_equal(got[0], x.want[0]), np.testing.assert_array_equal(got[1], x.want[1])
    finally:
        x.eng.close()
    x = Loaded()
    try:
        assert x.eng.pool_session_capacity == 0
        lib, eng = x.eng._lib, x.eng
        wide = hand_batch(chargers=((0, 1, 3),) * 2600, sessions=(((5, 1, 4), (5, 3, 6)), ()), T=8)
        assert lib.ev2g_load_scenarios(eng._h, C.byref(wide.to_c())) == ARG and eng.last_error() == NO_PORT
        wide = hand_batch(chargers=((0, 1, 3),) * 2600, sessions=(((5, 1, 4), (5, 5, 6)), ()), T=8)
        assert lib.ev2g_load_scenarios(eng._h, C.byref(wide.to_c())) == ARG
        assert eng.last_error() == PRE + "ports per env exceed the LDS staging capacity (P <= ~2400)"
        assert lib.ev2g_step(eng._h, x.acts.ptr, None, None, None, None) == STATE
    finally:
        x.eng.close()


# ---- routing ----------------------------------------------------------------------------------------------------------------------------------
WAVE = "ev2g_step_wave<2,0>"
OUTSIDE = "ports per env outside 2..64"
ROUTES = [   # (id, batch, engine arguments, switches, kernel_name, fallback_reason, big_kernel_reason)
    ("p1", lambda: spread(1), {}, {}, "ev2g_step_v2<256>", OUTSIDE, ""),
    ("p2", lambda: spread(2), {}, {}, WAVE, "", ""),
    ("p64", lambda: spread(64), {}, {}, WAVE, "", ""),
    ("p65", lambda: spread(65), {}, {}, "ev2g_step_v2<256>", OUTSIDE, ""),
    ("p2_pst", lambda: spread(2), dict(state="PublicPST", reward="SquaredTrackingErrorReward"), {}, "ev2g_step_wave<1,1>", "", ""),
    ("p2_loads", lambda: spread(2), dict(state="V2G_profit_max_loads", reward="profit_maximization"), {}, "ev2g_step_wave<0,2>", "", ""),
    ("two_transformers", lambda: hand_batch(chargers=((0, 1, 3), (1, 1, 3), (0, 1, 1), (1, 1, 3)), R=2), {}, {}, "ev2g_step_v2<256>", "more than one transformer", ""),
    ("two_ports_per_charger", lambda: hand_batch(chargers=((0, 2, 3), (0, 2, 3))), {}, {}, "ev2g_step_v2<256>", "multi-port chargers", ""),
    ("topology", lambda: hand_batch(chargers=((0, 2, 3), (0, 1, 3))), {}, {}, "ev2g_step_kernel", "chargers with different port counts (topology file)", ""),
    ("kernel_v2", lambda: spread(2), {}, {"EV2G_KERNEL": "v2"}, "ev2g_step_v2<256>", "EV2G_KERNEL=v2", ""),
    ("kernel_other", lambda: spread(2), {}, {"EV2G_KERNEL": "wave"}, WAVE, "", ""),
    ("no_dict", lambda: spread(2), {}, {"EV2G_NO_DICT": "1"}, WAVE, "", ""),
    ("no_big_small_env", lambda: spread(65), {}, {"EV2G_NO_BIG": "1"}, "ev2g_step_v2<256>", OUTSIDE, ""),
    ("p513", lambda: spread(513), dict(state="V2G_profit_max_loads"), {}, "ev2g_step_v2<1024>", OUTSIDE, ""),
    ("p1024", lambda: spread(1024), dict(state="V2G_profit_max_loads"), {}, "ev2g_step_v2<1024>", OUTSIDE, ""),
    ("p513_no_big", lambda: spread(513), dict(state="V2G_profit_max_loads"), {"EV2G_NO_BIG": "1"}, "ev2g_step_v2<1024>", OUTSIDE, "EV2G_NO_BIG is set"),
    ("p513_other_state", lambda: spread(513), {}, {}, "ev2g_step_v2<1024>", OUTSIDE, "the state function is not V2G_profit_max_loads"),
]


@pytest.mark.parametrize("name,batch,kw,env,kernel,fallback,big", ROUTES, ids=[r[0] for r in ROUTES])
def test_routing_table(monkeypatch, name, batch, kw, env, kernel, fallback, big):
    for k in ("EV2G_KERNEL", "EV2G_NO_DICT", "EV2G_NO_BIG", "EV2G_NO_FULL", "EV2G_NO_WIDE", "EV2G_NO_STRIDED", "EV2G_NO_INLAUNCH_STATS", "EV2G_POOL_SESSION_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (the facade's "not the fast path" warning)
        eng = engine(batch(), **kw)
    try:
        assert (eng.kernel_name, eng.fallback_reason, eng.big_kernel_reason) == (kernel, fallback, big)
        assert eng.last_launch_specialisation == -1 and eng.last_stats_route == -1
        if name.startswith("p513") or name == "p1024":   # the specialised launch: ev2g_step_big (5) where it routes, else ev2g_step_v2<1024, 1> / the general one
            assert launch(eng) == (5 if big == "" else 1 if "EV2G_NO_BIG" in big else 0)
    finally:
        eng.close()


def test_the_dictionary_switch_leaves_the_trajectory_alone(monkeypatch):
    """EV2G_NO_DICT (one ClsRec per session instead of the dictionary): the same numbers, bit for bit."""
    batch = hand_batch()
    eng = engine(batch)
    monkeypatch.setenv("EV2G_NO_DICT", "1")
    flat = engine(batch)
    monkeypatch.delenv("EV2G_NO_DICT")
    try:
        for a, b in zip(episode(eng), episode(flat)):
            np.testing.assert_array_equal(a, b)
    finally:
        eng.close(), flat.close()


@pytest.mark.parametrize("switch,stride0,strided", [(None, 2, 3), ("EV2G_NO_FULL", 0, 0), ("EV2G_NO_WIDE", 1, 0), ("EV2G_NO_STRIDED", 2, 0)])
def test_launch_specialisation_under_each_switch(monkeypatch, switch, stride0, strided):
    for k in ("EV2G_NO_FULL", "EV2G_NO_WIDE", "EV2G_NO_STRIDED"):
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    eng = engine(spread(4), state="PublicPST", reward="SquaredTrackingErrorReward")
    if switch:
        monkeypatch.delenv(switch)   # read when the scenarios are loaded, not at the launch
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (the facade's "general instantiation" warning)
            assert launch(eng) == stride0
            assert launch(eng, strided=True) == strided
        if switch == "EV2G_NO_FULL":
            why = (eng._lib.ev2g_last_launch_general_reason(eng._h) or b"").decode()
            assert why == "EV2G_NO_FULL is set (or the batch has more than 4094 efficiency tables)"
    finally:
        eng.close()


def test_statistics_reason_without_the_in_launch_phase(monkeypatch):
    monkeypatch.setenv("EV2G_NO_INLAUNCH_STATS", "1")
    eng = engine(spread(4), state="PublicPST", reward="SquaredTrackingErrorReward")
    monkeypatch.delenv("EV2G_NO_INLAUNCH_STATS")
    other = engine(spread(4), state="PublicPST", reward="SquaredTrackingErrorReward")
    try:
        for e in (eng, other):
            assert launch(e, e.T) == 2
        a, b = eng.stats(), other.stats()
        np.testing.assert_array_equal(a, b)
        assert (eng.last_stats_route, eng.last_stats_reason) == (0, "EV2G_NO_INLAUNCH_STATS is set")
        assert other.last_stats_route in (0, 1) and "EV2G_NO_INLAUNCH_STATS" not in other.last_stats_reason
    finally:
        eng.close(), other.close()


def test_a_second_batch_in_between_leaves_no_trace():
    """Load A, load a different B (other port count, two transformers, multi-port chargers, other state width), load A again: A's
    trajectory is the first load's, bit for bit -- on the fast path and through the general kernel."""
    import warnings
    a = hand_batch(seed=1)
    bs = [hand_batch(chargers=((0, 2, 3), (1, 1, 1), (0, 1, 3)), sessions=(((0, 1, 4), (0, 2, 9), (2, 3, 5), (0, 5, 7)), (), ((1, 2, 2), (1, 3, 8))), R=2, T=12, seed=2),
          spread(5, T=8, M=3)]
    eng = engine(a)
    try:
        first = episode(eng)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for b in bs:
                eng.load(b)
                assert (eng.P, eng.T, eng.E) == (b.n_ports, b.n_steps, b.n_envs)
                other = episode(eng)
                assert np.isfinite(other[1]).all()
                eng.load(a)
                again = episode(eng)
                np.testing.assert_array_equal(first[0], again[0]), np.testing.assert_array_equal(first[1], again[1])
    finally:
        eng.close()
