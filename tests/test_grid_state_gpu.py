"""V2G_grid_state, the grid statistics and the grid rollout on the device (csrc/ev2g_grid.h: ev2g_grid_state_kernel, the accumulators of
ev2g_grid_kernel<true>; ev2g_grid_state_attach / _observe / _run_observed / _rollout / _get_stats; EV2GymVec(state_function="V2G_grid_state",
grid_statistics=True)).

The state rows are held BIT FOR BIT to ev2gym_amd.grid.grid_state_numpy (held to the reference's own rows by tests/test_grid_state_cpu.py), fed
from ev2g_peek, the scenario arrays and the base profiles: the kernel copies and subtracts integers, nothing else.  Two batches: the 5-env,
33-port one of tests/test_grid_gpu.py, and 65 envs (one past a 64-row boundary) of 40 two-port chargers on 33 transformers -- P = 80, so a
row's port block crosses a wavefront, and chargers 33 .. 39 share transformers 0 .. 6 with chargers 0 .. 6, so the transformer-major slot
order differs from the reference's port order (port_slot is not the identity).
Counts of the accumulators are exact; their two float64 sums are held to 1e-9 of max(1, |value|), the project's bar."""
import datetime

import numpy as np
import pytest

from tests.test_grid_cpu import TOL, network, rel
from tests.test_grid_gpu import T_RUN, _actions, run_batch, run_profiles
from tests.test_heuristics_gpu import _engine

pytestmark = pytest.mark.gpu

KINDS = ("V2G_profitmaxV2", "V2G_profit_max")
WEIGHTS = (1.0, 50000.0)                       # Grid_V2G_profitmaxV2
START = datetime.datetime(2022, 1, 16, 22, 0)  # Sunday 22:00, 15-minute steps: step counter 8 is Monday 00:00


def wide_batch():
    """65 envs, 40 two-port chargers on 33 transformers (charger i on transformer i mod 33), 8 steps, run_batch's short-stay tables."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    tabs = dict(arrival_week=np.full(96, 60.0), arrival_weekend=np.full(96, 60.0), stay=np.full(48, 0.1), energy=np.full(48, 12.0), pv=np.full(8760, 0.3))
    b = generate(GenConfig.v2g_profit_plus_loads(65, 40, 33, seed=12, simulation_length=T_RUN, spawn_multiplier=4, hour=9, ev_min_time_of_stay=15,
                                                 number_of_ports_per_cs=2, data_tables=tabs))
    assert b.n_sessions >= 15 * 65
    return b


LIGHT_STEPS = (1, 2, 6)


def state_profiles(net, M, T):
    """run_profiles' seeded days with three steps lightened to 15 % of their load.  run_profiles alone puts a bus below 0.95 p.u. in EVERY
    step of every env (|v| down to 0.75), and the statistics need steps on both sides: with these rows steps 1, 2 and 6 stay inside the band
    whatever the chargers do (|v| >= 0.97 with 25 kW drawn at every bus) and the other five violate it."""
    load, pv = run_profiles(net, M, T)
    load = load.copy()
    load[:, list(LIGHT_STEPS)] = np.round(load[:, list(LIGHT_STEPS)] * 0.15, 1)
    return load, pv


class Ctx:
    """An engine with a grid and an attached state, and the host-side restatement of its rows."""

    def __init__(self, batch, starts=START, **kw):
        from ev2gym_amd.grid import time_features
        self.net = network(34)
        self.eng = eng = _engine(batch, KINDS, **kw)
        self.p_base, self.q_base = self.net.base_profiles(*state_profiles(self.net, eng.M, eng.T))
        self.g = eng.grid_create(self.net, (self.p_base, self.q_base), TOL, 100)
        ts = eng.batch.timescale
        self.tf = time_features(starts, ts, eng.T) if isinstance(starts, datetime.datetime) else np.stack([time_features(d, ts, eng.T) for d in starts])
        self.Dg = eng.grid_state_attach(self.g, self.tf)
        assert self.Dg == 6 + 2 * 33 + 3 * eng.P == eng.grid_state_dim(self.g)
        self.acts = _actions(eng, eng.T)
        self.d_act = eng.empty((eng.T, eng.E, eng.P)).upload(self.acts)

    def want_rows(self, offset=None):
        """grid_state_numpy of every env at the engine's step counter, from ev2g_peek and the host's copies of the scenario."""
        from ev2gym_amd.grid import grid_state_numpy
        eng, a = self.eng, self.eng.batch.arrays
        c, T = eng.current_step, eng.T
        off = eng.scenario_offset if offset is None else offset
        bus = np.repeat(a["cs_transformer"], a["cs_n_ports"])
        rows, occupied = [], []
        for e in range(eng.E):
            scn = (e + off) % eng.M
            pk = eng.peek(e)
            sess = pk["port_session"]
            dep = a["ev_t_dep"][a["env_session_start"][scn] + np.maximum(sess, 0)]
            cap = np.where(sess >= 0, pk["port_capacity"], np.nan)
            tf = self.tf[c] if self.tf.ndim == 2 else self.tf[scn, c]
            rows.append(grid_state_numpy(c, T, tf, a["charge_price"][scn], a["power_setpoints"][scn], pk["power_usage"], self.p_base[scn],
                                         self.q_base[scn], cap, dep, bus))
            occupied.append(sess >= 0)
        return np.array(rows), np.array(occupied)

    def step(self, t, **kw):
        E, P = self.eng.E, self.eng.P
        self.eng.grid_run(self.g, 1, None, self.d_act.at(t * E * P), 0, base_weight=WEIGHTS[0], voltage_weight=WEIGHTS[1], **kw)


@pytest.fixture(scope="module", params=["narrow", "wide"])
def ctx(request):
    c = Ctx(run_batch() if request.param == "narrow" else wide_batch())
    if request.param == "narrow":
        assert c.eng.kernel_name == "ev2g_step_v2<256>" and (c.eng.E, c.eng.P) == (5, 33)
    else:
        assert (c.eng.E, c.eng.P, c.eng.R, c.eng.C) == (65, 80, 33, 40)
    yield c
    c.eng.close()


def test_state_after_reset_after_every_step_and_after_the_last_step(ctx):
    """Counters 0 .. T; the three output modes (float64 only, float32 only, both) take turns, counter 0 and T get all three."""
    eng, g = ctx.eng, ctx.g
    o64, o32 = eng.empty((eng.E, ctx.Dg)), eng.empty((eng.E, ctx.Dg), np.float32)
    eng.reset()
    occupied, empty, priced = 0, 0, False
    for c in range(eng.T + 1):
        want, occ = ctx.want_rows()
        occupied, empty = occupied + int(occ.sum()), empty + int((~occ).sum())
        priced |= bool((want[:, 3] != 0).any())
        for mode in ((0, 1, 2) if c in (0, eng.T) else (c % 3,)):
            o64.upload(np.full((eng.E, ctx.Dg), -7.0)), o32.upload(np.full((eng.E, ctx.Dg), -7.0, np.float32))
            eng.grid_observe(g, o64 if mode != 1 else None, o32 if mode != 0 else None)
            eng.synchronize()
            got64, got32 = o64.to_host(), o32.to_host()
            if mode != 1:
                assert np.array_equal(got64, want), (c, mode, np.argwhere(got64 != want)[:5])
            else:
                assert (got64 == -7.0).all()
            if mode != 0:
                assert np.array_equal(got32, np.float32(want)), (c, mode)
            else:
                assert (got32 == -7.0).all()
        if c == 0:
            assert (want[:, 5] == 0).all()
        if c == eng.T:
            assert (want[:, 3:5] == 0).all() and np.array_equal(want[:, 1:3], np.tile([0.0, 1.0], (eng.E, 1)))   # Monday 00:00
        else:
            ctx.step(c)
    assert occupied and empty and priced
    for b in (o64, o32):
        b.free()


def test_run_observed_equals_grid_run_and_writes_the_next_counters_state(ctx):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    eng, g = ctx.eng, ctx.g
    E, P, T, Dg, nb = eng.E, eng.P, eng.T, ctx.Dg, 34
    bw, vw = WEIGHTS

    def bufs():
        return dict(reward=eng.empty((T, E)), done=eng.empty((T, E), np.uint8), mask=eng.empty((T, E, P), np.uint8), vm=eng.empty((T, E, nb)))

    def strides(b, k0=0):
        return dict(reward=b["reward"].at(k0 * E), r_stride=E, done=b["done"].at(k0 * E), d_stride=E, mask=b["mask"].at(k0 * E * P), m_stride=E * P,
                    vm=b["vm"].at(k0 * E * nb), v_stride=E * nb, base_weight=bw, voltage_weight=vw)

    # the rows to expect, counter by counter, along a plain grid_run
    plain = bufs()
    eng.reset()
    rows = []
    for t in range(T):
        eng.grid_run(g, 1, None, ctx.d_act.at(t * E * P), 0, reward=plain["reward"].at(t * E), done=plain["done"].at(t * E),
                     mask=plain["mask"].at(t * E * P), vm=plain["vm"].at(t * E * nb), base_weight=bw, voltage_weight=vw)
        rows.append(ctx.want_rows()[0])
    rows = np.array(rows)
    plain = {k: v.to_host() for k, v in plain.items()}
    # one segment, strided float64 and float32 rows
    one, gobs, gobs32 = bufs(), eng.empty((T, E, Dg)), eng.empty((T, E, Dg), np.float32)
    eng.reset()
    eng.grid_run_observed(g, T, None, ctx.d_act, E * P, gobs=gobs, go_stride=E * Dg, gobs32=gobs32, go32_stride=E * Dg, **strides(one))
    for k in plain:
        assert np.array_equal(one[k].to_host(), plain[k]), k
    assert np.array_equal(gobs.to_host(), rows) and np.array_equal(gobs32.to_host(), np.float32(rows))
    with pytest.raises(EngineError) as ei:
        eng.grid_run_observed(g, 1, None, ctx.d_act, 0, gobs=gobs)
    assert ei.value.code == _abi.ERR_DONE
    # two segments (3 + 5), stride 0 for the rows: the block holds the last counter's
    two, last = bufs(), eng.empty((E, Dg))
    eng.reset()
    eng.grid_run_observed(g, 3, None, ctx.d_act, E * P, gobs=last, go_stride=0, **strides(two))
    assert np.array_equal(last.to_host(), rows[2])
    eng.grid_run_observed(g, T - 3, None, ctx.d_act.at(3 * E * P), E * P, gobs=last, go_stride=0, **strides(two, 3))
    assert np.array_equal(last.to_host(), rows[T - 1])
    for k in plain:
        assert np.array_equal(two[k].to_host(), plain[k]), k
    eng.check_faults()
    for b in list(one.values()) + list(two.values()) + [gobs, gobs32, last]:
        b.free()


def test_state_follows_the_pool_window():
    """Three envs on five scenarios, reset(offset=4): env e reads scenario (e + 4) mod 5 -- its prices, setpoints, base profiles and, with one
    starting date per scenario, its time features."""
    starts = [START + datetime.timedelta(days=d, hours=d) for d in range(5)]
    c = Ctx(run_batch(), starts=starts, n_active_envs=3)
    eng = c.eng
    assert (eng.E, eng.M) == (3, 5) and c.tf.shape == (5, eng.T + 1, 3)
    o64 = eng.empty((eng.E, c.Dg))
    eng.reset(offset=4)
    for t in range(eng.T + 1):
        eng.grid_observe(c.g, o64)
        got, want, other = o64.to_host(), c.want_rows()[0], c.want_rows(offset=0)[0]
        assert np.array_equal(got, want), t
        lo, hi = (3, 6 + 2 * 33) if t < eng.T else (6, 6 + 2 * 33)   # (the price and the setpoint are 0 for every scenario at the end)
        assert (got[:, lo:hi] != other[:, lo:hi]).any(axis=1).all() and (got[:, 0:3] != other[:, 0:3]).any(axis=1).all(), t
        if t < eng.T:
            c.step(t)
    eng.close()


def _episode(ctx, acts_dev, splits):
    """One episode through grid_run in the given segments: (vm [T, E, n_bus], reward [T, E], the grid's statistics)."""
    eng, g = ctx.eng, ctx.g
    E, P, T = eng.E, eng.P, eng.T
    vm, rew = eng.empty((T, E, 34)), eng.empty((T, E))
    eng.reset()
    t = 0
    for k in splits:
        eng.grid_run(g, k, None, acts_dev.at(t * E * P), E * P, reward=rew.at(t * E), r_stride=E, vm=vm.at(t * E * 34), v_stride=E * 34,
                     base_weight=WEIGHTS[0], voltage_weight=WEIGHTS[1])
        t += k
    out = vm.to_host(), rew.to_host(), eng.grid_get_stats(g)
    vm.free(), rew.free()
    return out


def _check_stats(stats, vm, rew):
    from ev2gym_amd.grid import voltage_statistics
    for e in range(vm.shape[1]):
        total, count, steps = voltage_statistics(vm[:, e])
        assert stats["voltage_violation_counter"][e] == count and stats["voltage_violation_counter_per_step"][e] == steps, e
        assert abs(stats["voltage_violation"][e] - total) <= 1e-9 * max(1.0, abs(total)), e
        assert abs(stats["total_reward"][e] - rew[:, e].sum()) <= 1e-9 * max(1.0, abs(rew[:, e].sum())), e


def test_accumulators_hold_the_episodes_voltage_statistics(ctx):
    from ev2gym_amd.grid import solve_numpy, voltage_statistics
    eng, net = ctx.eng, ctx.net
    E, P, T = eng.E, eng.P, eng.T
    vm, rew, stats = _episode(ctx, ctx.d_act, (T,))
    assert stats["voltage_violation_counter"].dtype == np.int32
    _check_stats(stats, vm, rew)
    assert stats["voltage_violation_counter"].max() > 0 and stats["voltage_violation"].min() < 0
    # against the numpy solver on the same node powers: exact counts, given that no |v| of the reference run sits on a band edge
    eng.reset()
    scn = (np.arange(E) + eng.scenario_offset) % eng.M
    ref = np.empty((T, E, 34))
    for t in range(T):
        ctx.step(t)
        tr = np.array([eng.peek(e)["tr_power"] for e in range(E)])
        ref[t] = solve_numpy(net.K, net.L, ctx.p_base[scn, t] + tr, ctx.q_base[scn, t], net.s_base, TOL, 100)["vm"]
    assert np.minimum(np.abs(ref - 0.95), np.abs(ref - 1.05)).min() > 1e-9
    bad = ((ref < 0.95) | (ref > 1.05)).any(axis=-1)
    print("violating (step, env) pairs", int(bad.sum()), "of", bad.size)
    assert bad.any() and (~bad).any() and not bad[list(LIGHT_STEPS)].any()
    for e in range(E):
        _, count, steps = voltage_statistics(ref[:, e])
        assert stats["voltage_violation_counter"][e] == count and stats["voltage_violation_counter_per_step"][e] == steps, e
    again = eng.grid_get_stats(ctx.g)   # (the stepwise episode just run: the same values, one launch per call)
    for k in stats:
        assert np.array_equal(again[k], stats[k]), k
    # a second episode with other actions reports that episode only; a 3 + 5 split reports what the unsplit run does
    quiet = eng.empty((T, E, P)).upload(np.zeros((T, E, P)))
    vm2, rew2, stats2 = _episode(ctx, quiet, (T,))
    _check_stats(stats2, vm2, rew2)
    assert not np.array_equal(stats2["total_reward"], stats["total_reward"])
    vm3, rew3, stats3 = _episode(ctx, ctx.d_act, (3, 5))
    assert np.array_equal(vm3, vm) and np.array_equal(rew3, rew)
    for k in stats:
        assert np.array_equal(stats3[k], stats[k]), k
    quiet.free()


def test_rollout_equals_the_hand_made_chain(ctx):
    from ev2gym_amd import _abi
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import EngineError
    eng, g = ctx.eng, ctx.g
    E, P, T, Dg, nb = eng.E, eng.P, eng.T, ctx.Dg, 34
    bw, vw = WEIGHTS
    mlp = eng.mlp_create(*init_mlp_weights(Dg, P, seed=9, h1=32, h2=32), out_lo=-1.0, precision="bf16")
    rew, done, mask, vm = eng.empty((T, E)), eng.empty((T, E), np.uint8), eng.empty((T, E, P), np.uint8), eng.empty((T, E, nb))
    eng.reset()
    with pytest.raises(EngineError) as ei:   # nothing has filled the grid's float32 row for this episode's counter 0
        eng.grid_rollout(g, mlp, 1, rew, E, done, E, mask, E * P, vm, E * nb, bw, vw)
    assert ei.value.code == _abi.ERR_STATE
    eng.grid_observe(g)
    eng.grid_rollout(g, mlp, 3, rew, E, done, E, mask, E * P, vm, E * nb, bw, vw)
    eng.grid_rollout(g, mlp, T - 3, rew.at(3 * E), E, done.at(3 * E), E, mask.at(3 * E * P), E * P, vm.at(3 * E * nb), E * nb, bw, vw)
    got = dict(rew=rew.to_host(), done=done.to_host(), mask=mask.to_host(), vm=vm.to_host(), stats=eng.grid_get_stats(g))
    assert got["done"][T - 1].all() and not got["done"][:T - 1].any()
    with pytest.raises(EngineError) as ei:
        eng.grid_rollout(g, mlp, 1, rew, E, done, E, mask, E * P, vm, E * nb, bw, vw)
    assert ei.value.code == _abi.ERR_DONE
    # a step outside the grid's calls invalidates the row even though the counter matches again
    eng.reset()
    eng.grid_observe(g)
    eng.reset()
    with pytest.raises(EngineError) as ei:
        eng.grid_rollout(g, mlp, 1, rew, E, done, E, mask, E * P, vm, E * nb, bw, vw)
    assert ei.value.code == _abi.ERR_STATE
    wrong = eng.mlp_create(*init_mlp_weights(Dg, P + 1, seed=9, h1=32, h2=32), out_lo=-1.0)
    eng.grid_observe(g)
    with pytest.raises(EngineError) as ei:
        eng.grid_rollout(g, wrong, 1, rew, E, done, E, mask, E * P, vm, E * nb, bw, vw)
    assert ei.value.code == _abi.ERR_ARG
    # the chain by hand: observe -> forward -> widen (on the host: float32 -> float64 is exact) -> one observed step
    x32, a32, a64 = eng.empty((E, Dg), np.float32), eng.empty((E, P), np.float32), eng.empty((E, P))
    r1, d1, m1, v1 = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8), eng.empty((E, nb))
    eng.reset()
    eng.grid_observe(g, None, x32)
    moved = False
    for t in range(T):
        eng.mlp_forward(mlp, x32, a32, E)
        eng.synchronize()
        act = a32.to_host()
        moved |= bool((act != act[0, 0]).any())
        a64.upload(act.astype(np.float64))
        eng.grid_run_observed(g, 1, None, a64, 0, None, 0, r1, 0, d1, 0, m1, 0, v1, 0, bw, vw, gobs32=x32)
        for k, b in (("rew", r1), ("done", d1), ("mask", m1), ("vm", v1)):
            assert np.array_equal(b.to_host(), got[k][t]), (k, t)
    assert moved
    chain = eng.grid_get_stats(g)
    for k in chain:
        assert np.array_equal(chain[k], got["stats"][k]), k
    eng.check_faults()
    eng.mlp_destroy(mlp), eng.mlp_destroy(wrong)
    for b in (rew, done, mask, vm, x32, a32, a64, r1, d1, m1, v1):
        b.free()


def test_vec_env_returns_grid_rows_and_fills_the_grid_statistics():
    from ev2gym_amd import _abi
    from ev2gym_amd.vec_env import EV2GymVec
    net, batch = network(34), run_batch()
    load, pv = state_profiles(net, batch.n_envs, T_RUN)
    kw = dict(scenarios=batch, reward_function="V2G_profitmaxV2", use_torch=False)
    gkw = dict(grid=net, grid_profiles=(load, pv), grid_reward="Grid_V2G_profitmaxV2")
    env = EV2GymVec(state_function="V2G_grid_state", grid_start=START, grid_statistics=True, **gkw, **kw)
    off = EV2GymVec(state_function="V2G_profit_max", **gkw, **kw)          # the flag left off
    plain = EV2GymVec(state_function="V2G_profit_max", **kw)
    Dg = 6 + 2 * 33 + 3 * 33
    assert env.obs_dim == Dg and env.observation_space.shape == (Dg,)
    ctx = Ctx.__new__(Ctx)   # the host-side restatement on the env's own engine
    ctx.eng, ctx.net = env.engine, net
    ctx.p_base, ctx.q_base = net.base_profiles(load, pv)
    from ev2gym_amd.grid import time_features
    ctx.tf = time_features(START, batch.timescale, T_RUN)
    obs, _ = env.reset(seed=env.seed)
    off.reset(seed=env.seed), plain.reset(seed=env.seed)
    assert obs.shape == (env.num_envs, Dg) and np.array_equal(obs, ctx.want_rows()[0])
    acts, total = _actions(env.engine, T_RUN), np.zeros(env.num_envs)
    for t in range(T_RUN):
        obs, rew, done, _, info = env.step(acts[t])
        _, rew1, _, _, info1 = off.step(acts[t])
        _, _, _, _, info0 = plain.step(acts[t])
        assert obs.shape == (env.num_envs, Dg) and np.array_equal(obs, ctx.want_rows()[0]), t
        assert np.array_equal(rew, rew1)
        total += rew
    assert done.all() and set(info) == set(info0) == set(info1)
    from ev2gym_amd.grid import voltage_statistics
    assert rel(info["total_reward"], total) <= 1e-9 and not np.array_equal(info["total_reward"], info0["total_reward"])
    assert info["voltage_violation_counter"].max() > 0 and info["voltage_violation_counter_per_step"].max() > 0 and info["voltage_violation"].min() < 0
    assert not np.asarray(info["saved_grid_energy"]).any()
    _, count, steps = voltage_statistics(env.node_voltage[0][None])   # the last step's row is part of the counts
    assert (info["voltage_violation_counter"][0] >= count) and (info["voltage_violation_counter_per_step"][0] >= steps)
    for k in info0:   # without the flag: the plain env's info, as before
        if k not in ("action_mask", "cost"):
            assert np.array_equal(info1[k], info0[k], equal_nan=True), k
    for k in _abi.STAT_NAMES[:-1]:
        assert np.array_equal(info[k], info0[k], equal_nan=True), k
    for e in (env, off, plain):
        e.close()
