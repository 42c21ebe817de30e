"""The distribution grid's power flow on the device (csrc/ev2g_grid.h, ev2g_grid_*; the reference's models/grid.py and
models/grid_utility/grid_tensor.py): the batched solver against the reference's own solutions (the grid fixtures) and against the numpy
restatement ev2gym_amd.grid.solve_numpy (held to the reference by tests/test_grid_cpu.py), then through ev2g_grid_run and EV2GymVec.

Bars: voltages, |v| and the voltage loss within 1e-9 of max(1, |reference|), the project's parity bar (the kernel sums K lambda in another
order than BLAS does: rounding-level differences, a few 1e-16 per term, iterated at most 100 times with a contraction); iteration counts
exactly equal (the fixtures keep no case whose residual is within 1e-3 of the tolerance, and the seeded random rows are filtered the same way)."""
import numpy as np
import pytest

from tests.test_grid_cpu import NETWORKS, TOL, fixture, network, rel
from tests.test_heuristics_gpu import _engine

pytestmark = pytest.mark.gpu

KINDS = ("profit_maximization", "V2G_profit_max")
ROWS = (1, 3, 65, 130)   # a lone env, a ragged workgroup (four rows each), one past a workgroup / 64-row boundary, and two of them


@pytest.fixture(scope="module")
def host():
    """A small engine whose handle owns the solver-only grids (the solver reads no engine state)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    eng = _engine(generate(GenConfig.v2g_profit_plus_loads(2, 4, 1, seed=3, simulation_length=8)), KINDS)
    yield eng
    eng.close()


def _solve(eng, g, P, Q, n_bus, want_v=True):
    rows, n = P.shape
    dp, dq = eng.empty((rows, n)).upload(P), eng.empty((rows, n)).upload(Q)
    vm, vc, it, lv = eng.empty((rows, n_bus)), eng.empty((rows, n, 2)), eng.empty((rows,), np.int32), eng.empty((rows,))
    eng.grid_solve(g, dp, dq, rows, vm, vc if want_v else None, it, lv)
    eng.synchronize()
    out = dict(vm=vm.to_host(), iters=it.to_host(), loss_v=lv.to_host())
    if want_v:
        c = vc.to_host()
        out["v"] = c[..., 0] + 1j * c[..., 1]
    for b in (dp, dq, vm, vc, it, lv):
        b.free()
    return out


def _check(got, want, what):
    from ev2gym_amd.grid import voltage_loss
    errs = dict(vm=rel(got["vm"], want["vm"]), re=rel(got["v"].real, want["v"].real), im=rel(got["v"].imag, want["v"].imag),
                loss=rel(got["loss_v"], voltage_loss(want["vm"])))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()}, "iters", sorted(set(got["iters"].tolist())))
    assert np.array_equal(got["iters"], want["iters"]), what
    assert max(errs.values()) <= 1e-9, (what, errs)
    assert np.abs(got["vm"] / want["vm"] - 1.0).max() <= 1e-9, what   # |v| is near 1: a true relative bar
    # the slack bus in front; |v| of the voltages written next to it (hypot on either side: an ulp or two)
    assert np.array_equal(got["vm"][:, 0], np.ones(len(got["vm"]))) and rel(got["vm"][:, 1:], np.abs(got["v"])) <= 1e-15


def _random_rows(z, n_rows, seed):
    """Seeded loads of the fixtures' range (0.3 .. 3 x nominal, EV injections of +-22 kW per bus), filtered by the fixtures' guard: no row whose
    last two residuals lie within 1e-3 of the tolerance."""
    from ev2gym_amd.grid import solve_numpy
    rng, n = np.random.default_rng(seed), z["K"].shape[0]
    nominal = network(n + 1).p_values[1:]
    P = nominal * rng.uniform(0.3, 3.0, (2 * n_rows, 1)) * rng.uniform(0.8, 1.2, (2 * n_rows, n)) + rng.uniform(-22, 22, (2 * n_rows, n))
    Q = np.round(P * z["pf"], 1)
    ref = solve_numpy(z["K"], z["L"], P, Q, 1000, TOL, 100, residuals=True)
    keep = np.flatnonzero((np.abs(ref["res"] - TOL) > 1e-3 * TOL).all(axis=1) & (ref["iters"] < 100))[:n_rows]
    assert len(keep) == n_rows
    return P[keep], Q[keep], {k: v[keep] for k, v in ref.items()}


@pytest.mark.parametrize("n_bus", NETWORKS)
def test_solver_reproduces_the_reference_and_the_numpy_restatement(host, n_bus):
    """33 rows per column (no multiple of 16 or 64) and 122 (two lanes' worth per wavefront), every row count; neighbouring rows carry fixture
    cases of different iteration counts, so a row that has converged sits next to rows that go on."""
    z = fixture(n_bus)
    g = host.grid_create(type("Net", (), dict(n_bus=n_bus, K=z["K"], L=z["L"], s_base=float(z["s_base"])))(), None, TOL, 100)
    nc = len(z["iters"])
    for rows in ROWS:
        idx = np.arange(rows) % nc
        assert rows == 1 or (z["iters"][idx][1:] != z["iters"][idx][:-1]).mean() > 0.9
        want = dict(v=z["v"][idx], vm=z["vm"][idx], iters=z["iters"][idx])
        _check(_solve(host, g, z["P"][idx], z["Q"][idx], n_bus), want, f"{n_bus} buses, fixture x {rows}")
        P, Q, ref = _random_rows(z, rows, 100 + rows)
        _check(_solve(host, g, P, Q, n_bus), ref, f"{n_bus} buses, random x {rows}")
    # without the optional complex output
    got = _solve(host, g, z["P"], z["Q"], n_bus, want_v=False)
    assert np.array_equal(got["iters"], z["iters"]) and rel(got["vm"], z["vm"]) <= 1e-9
    host.grid_destroy(g)


@pytest.mark.parametrize("n_bus", NETWORKS)
def test_solver_stops_at_max_iter_on_zero_load_and_on_nan(host, n_bus):
    from ev2gym_amd.grid import solve_numpy
    z = fixture(n_bus)
    net = type("Net", (), dict(n_bus=n_bus, K=z["K"], L=z["L"], s_base=1000.0))()
    n, nc = n_bus - 1, len(z["iters"])
    idx = np.arange(65) % nc
    for cap in (0, 2):   # every row stops at the cap with the reference's v of that many iterations
        g = host.grid_create(net, None, TOL, cap)
        want = solve_numpy(z["K"], z["L"], z["P"][idx], z["Q"][idx], 1000, TOL, cap)
        assert (want["iters"] == np.minimum(z["iters"][idx], cap)).all()
        _check(_solve(host, g, z["P"][idx], z["Q"][idx], n_bus), want, f"{n_bus} buses, max_iter {cap}")
        host.grid_destroy(g)
    g = host.grid_create(net, None, TOL, 100)
    # a row of zero load between loaded ones: |v| = |L|, in the reference's count
    P, Q = z["P"][[1, 0, 2]].copy(), z["Q"][[1, 0, 2]].copy()
    P[1] = Q[1] = 0.0
    want = solve_numpy(z["K"], z["L"], P, Q, 1000, TOL, 100)
    got = _solve(host, g, P, Q, n_bus)
    _check(got, want, f"{n_bus} buses, zero load")
    assert rel(got["vm"][1, 1:], np.abs(z["L"])) <= 1e-15 * 4 and got["loss_v"][1] == want["loss_v"][1]
    # a NaN load ends its own row at once (numpy: `nan >= tolerance` is False) and leaves its neighbours alone
    P, Q = z["P"][[1, 2, 3]].copy(), z["Q"][[1, 2, 3]].copy()
    P[1, n // 2] = np.nan
    want = solve_numpy(z["K"], z["L"], P, Q, 1000, TOL, 100)
    got = _solve(host, g, P, Q, n_bus)
    assert np.array_equal(got["iters"], want["iters"]) and got["iters"][1] == 1 and np.isnan(got["loss_v"][1])
    assert rel(got["vm"][[0, 2]], want["vm"][[0, 2]]) <= 1e-9
    host.grid_destroy(g)


def test_create_refuses_what_the_reference_cannot_mean(host):
    from ev2gym_amd.engine import EngineError
    z = fixture(34)
    net = type("Net", (), dict(n_bus=34, K=z["K"], L=z["L"], s_base=1000.0))()
    prof = np.zeros((host.M, host.T + 1, 33))
    with pytest.raises(EngineError, match="transformers"):   # the host engine has one transformer
        host.grid_create(net, (prof, prof))
    with pytest.raises(EngineError, match="max_iter"):
        host.grid_create(net, None, TOL, -1)
    g = host.grid_create(net, None)
    act = host.empty((host.E, host.P))
    with pytest.raises(EngineError, match="without base profiles"):
        host.grid_run(g, 1, None, act)
    host.grid_destroy(g)
    act.free()


# ---- ev2g_grid_run / EV2GymVec on a 33-transformer engine --------------------------------------------------------------------------------

E_RUN, T_RUN = 5, 8


def run_batch():
    """33 one-port chargers, one transformer each (transformer i feeds bus i + 1), 8 steps.  The generator drops sessions that would outlast
    the episode, and its fitted stays are hours long: tables with six-minute stays and an arrival rate that fills two ports in three at the
    first spawn step give every env about twenty EVs that arrive at step 3 and leave at step 6."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    tabs = dict(arrival_week=np.full(96, 60.0), arrival_weekend=np.full(96, 60.0), stay=np.full(48, 0.1), energy=np.full(48, 12.0), pv=np.full(8760, 0.3))
    b = generate(GenConfig.v2g_profit_plus_loads(E_RUN, 33, 33, seed=11, simulation_length=T_RUN, spawn_multiplier=4, hour=9, ev_min_time_of_stay=15,
                                                 data_tables=tabs))
    assert b.n_sessions >= 15 * E_RUN
    return b


def run_profiles(net, M, T):
    """Seeded load / PV days per scenario, heavy enough that some buses leave the 5 % band (a loss of exactly 0 would hide the reward)."""
    rng = np.random.default_rng(5)
    load = np.round(net.p_values * rng.uniform(1.5, 2.6, (M, T + 1, net.n_bus)), 1)
    pv = np.round(net.p_values * rng.uniform(0.0, 0.3, (M, T + 1, net.n_bus)), 1)
    return load, pv


def _actions(eng, k):
    from ev2gym_amd.engine import host_uniform
    return host_uniform(k * eng.E * eng.P, 77, -1.0, 1.0).reshape(k, eng.E, eng.P)


@pytest.mark.parametrize("reward,weights", [("profit_maximization", (0.0, 1000.0)), ("V2G_profitmaxV2", (1.0, 50000.0))])
def test_grid_run_composes_step_and_power_flow(reward, weights):
    """Per step: vm and reward equal solve_numpy fed with that step's transformer powers (read back through ev2g_peek) on top of the base
    profiles; obs / done / mask are the plain run's, bit for bit; strided and stride-0 vm; EV2G_ERR_DONE past the end.  33 transformers rule
    out ev2g_step_wave (one transformer) and ev2g_step_big (more than 512 ports): the route is ev2g_step_v2<256>."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.grid import solve_numpy
    net, batch = network(34), run_batch()
    eng = _engine(batch, (reward, "V2G_profit_max"))
    assert eng.kernel_name == "ev2g_step_v2<256>" and eng.R == 33 and eng.P == 33
    E, P, D, T, n_bus = eng.E, eng.P, eng.D, eng.T, 34
    p_base, q_base = net.base_profiles(*run_profiles(net, eng.M, T))
    g = eng.grid_create(net, (p_base, q_base), TOL, 100)
    act = eng.empty((T, E, P)).upload(_actions(eng, T))
    bw, vw = weights

    # the plain run: every step's outputs, and the transformer powers after each step
    obs, rew, done, mask = eng.empty((T, E, D)), eng.empty((T, E)), eng.empty((T, E), np.uint8), eng.empty((T, E, P), np.uint8)
    eng.reset()
    tr = np.empty((T, E, 33))
    for t in range(T):
        eng.step_n(1, act.at(t * E * P), 0, obs.at(t * E * D), 0, rew.at(t * E), 0, done.at(t * E), 0, mask.at(t * E * P), 0, auto_reset=0)
        for e in range(E):
            tr[t, e] = eng.peek(e)["tr_power"]
    plain = dict(obs=obs.to_host(), rew=rew.to_host(), done=done.to_host(), mask=mask.to_host())
    assert np.abs(tr).max() > 5.0   # EVs did charge
    scn = (np.arange(E) + eng.scenario_offset) % eng.M
    want = [solve_numpy(net.K, net.L, p_base[scn, t] + tr[t], q_base[scn, t], net.s_base, TOL, 100) for t in range(T)]
    want_vm, want_loss = np.array([w["vm"] for w in want]), np.array([w["loss_v"] for w in want])
    assert (want_loss < 0).any()

    # the same steps through ev2g_grid_run, in two segments, strided vm
    vm = eng.empty((T, E, n_bus))
    eng.reset()
    k1 = 3
    eng.grid_run(g, k1, None, act, E * P, obs, E * D, rew, E, done, E, mask, E * P, vm, E * n_bus, bw, vw)
    eng.grid_run(g, T - k1, None, act.at(k1 * E * P), E * P, obs.at(k1 * E * D), E * D, rew.at(k1 * E), E, done.at(k1 * E), E,
                 mask.at(k1 * E * P), E * P, vm.at(k1 * E * n_bus), E * n_bus, bw, vw)
    got = dict(obs=obs.to_host(), rew=rew.to_host(), done=done.to_host(), mask=mask.to_host(), vm=vm.to_host())
    for k in ("obs", "done", "mask"):
        assert np.array_equal(got[k], plain[k]), k
    print("vm", rel(got["vm"], want_vm))
    assert rel(got["vm"], want_vm) <= 1e-9
    if bw == 0.0:
        # 1000 * loss_v exactly as composed: the device's own loss, recomputed from the voltages it wrote, within the sum's rounding
        assert rel(got["rew"], vw * want_loss) <= 1e-9
        dev_loss = np.minimum(0.0, 0.05 - np.abs(1 - got["vm"])).sum(axis=-1)
        assert np.abs(got["rew"] - vw * dev_loss).max() <= 1e-12 * vw
    else:
        assert np.abs(plain["rew"]).max() > 0
        assert rel(got["rew"], bw * plain["rew"] + vw * want_loss) <= 1e-9
    with pytest.raises(EngineError) as ei:
        eng.grid_run(g, 1, None, act, 0, obs, 0, rew, 0, done, 0, mask, 0, vm, 0, bw, vw)
    assert ei.value.code == _abi.ERR_DONE

    # stride 0: one block of every output, rewritten each step; and the grid's own vm / reward rows when the caller passes none
    eng.reset()
    eng.grid_run(g, T, None, act, E * P, obs, 0, rew, 0, done, 0, mask, 0, vm, 0, bw, vw)
    assert np.array_equal(vm.to_host()[0], got["vm"][T - 1]) and np.array_equal(rew.to_host()[0], got["rew"][T - 1])
    assert np.array_equal(obs.to_host()[0], plain["obs"][T - 1])
    eng.reset()
    eng.grid_run(g, T, None, act, E * P)
    eng.check_faults()
    # an agent in front of the step, as in ev2g_heuristic_run
    agent = eng.heuristic_create("ChargeAsFastAsPossibleToDesiredCapacity")
    eng.reset()
    eng.grid_run(g, T, agent, None, 0, obs, 0, rew, 0, done, 0, mask, 0, vm, 0, bw, vw)
    a_vm = vm.to_host()[0]
    tr_last = np.array([eng.peek(e)["tr_power"] for e in range(E)])
    w = solve_numpy(net.K, net.L, p_base[scn, T - 1] + tr_last, q_base[scn, T - 1], net.s_base, TOL, 100)
    assert rel(a_vm, w["vm"]) <= 1e-9
    eng.check_faults()
    eng.close()


def test_grid_run_follows_the_pool_window():
    """Three envs on a pool of five scenarios, reset onto the window that starts at scenario 4 and wraps: env e takes the base profiles of
    scenario (e + 4) mod 5, every scenario's profiles being different."""
    from ev2gym_amd.grid import solve_numpy
    net, batch = network(34), run_batch()
    eng = _engine(batch, ("profit_maximization", "V2G_profit_max"), n_active_envs=3)
    E, P, T = eng.E, eng.P, eng.T
    assert (E, eng.M) == (3, 5)
    p_base, q_base = net.base_profiles(*run_profiles(net, eng.M, T))
    g = eng.grid_create(net, (p_base, q_base), TOL, 100)
    act, vm, rew = eng.empty((T, E, P)).upload(_actions(eng, T)), eng.empty((T, E, 34)), eng.empty((T, E))
    eng.reset(offset=4)
    assert eng.scenario_offset == 4
    scn = (np.arange(E) + 4) % 5
    for t in range(T):
        eng.grid_run(g, 1, None, act.at(t * E * P), 0, reward=rew.at(t * E), vm=vm.at(t * E * 34), base_weight=0.0, voltage_weight=1000.0)
        tr = np.array([eng.peek(e)["tr_power"] for e in range(E)])
        w = solve_numpy(net.K, net.L, p_base[scn, t] + tr, q_base[scn, t], net.s_base, TOL, 100)
        assert rel(vm.to_host()[t], w["vm"]) <= 1e-9 and rel(rew.to_host()[t], 1000.0 * w["loss_v"]) <= 1e-9, t
        other = solve_numpy(net.K, net.L, p_base[np.arange(E), t] + tr, q_base[np.arange(E), t], net.s_base, TOL, 100)
        assert rel(other["vm"], w["vm"]) > 1e-6   # the window matters: offset 0's profiles give other voltages
    eng.check_faults()
    eng.close()


def test_vec_env_exposes_node_voltage_and_is_unchanged_without_a_grid():
    from ev2gym_amd.grid import solve_numpy
    from ev2gym_amd.vec_env import EV2GymVec
    net, batch = network(34), run_batch()
    load, pv = run_profiles(net, batch.n_envs, T_RUN)
    kw = dict(scenarios=batch, state_function="V2G_profit_max", reward_function="V2G_profitmaxV2", use_torch=False)
    env = EV2GymVec(grid=net, grid_profiles=(load, pv), grid_reward="Grid_V2G_profitmaxV2", **kw)
    plain = EV2GymVec(**kw)
    assert plain.node_voltage is None and env.node_voltage is None
    p_base, q_base = net.base_profiles(load, pv)
    acts = _actions(env.engine, T_RUN)
    scn = (np.arange(env.num_envs) + env.engine.scenario_offset) % env.engine.M
    assert env.engine.scenario_offset == plain.engine.scenario_offset
    for t in range(T_RUN):
        obs, rew, done, _, info = env.step(acts[t])
        obs0, rew0, done0, _, info0 = plain.step(acts[t])
        tr = np.array([plain.engine.peek(e)["tr_power"] for e in range(env.num_envs)])
        w = solve_numpy(net.K, net.L, p_base[scn, t] + tr, q_base[scn, t], net.s_base, TOL, 100)
        assert env.node_voltage.shape == (env.num_envs, 34) and rel(env.node_voltage, w["vm"]) <= 1e-9
        assert rel(rew, rew0 + 50000.0 * w["loss_v"]) <= 1e-9
        assert np.array_equal(obs, obs0) and np.array_equal(done, done0) and np.array_equal(info["action_mask"], info0["action_mask"])
    assert done.all() and set(info) == set(info0)
    for k in info0:
        if k not in ("action_mask", "cost"):
            assert np.array_equal(info[k], info0[k], equal_nan=True), k   # statistics keep the step kernel's reward
    with pytest.raises(ValueError, match="unknown grid_reward"):
        EV2GymVec(grid=net, grid_profiles=(load, pv), grid_reward="V2G_grid_full_reward", **kw)
    env.close()
    plain.close()
